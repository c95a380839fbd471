// f110_agents.hip — k_agents, the first launch of an env step (f110_step.cpp): one thread per car:
// reset/autoreset, RaceCar.update_pose (steer delay, pid, RK4 of vehicle_dynamics_st, clamps), scan
// pose, first EDT lookup, and the car's beam-index runs.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "../../include/f110.h"
#include "f110_beam_runs.h"
#include "f110_dynamics.h"
#include "f110_env_rows.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_rng.h"
#include "f110_sincos.h"
#include "f110_sincos_table.h"
#include "f110_spawn.h"
#include "f110_step_args.h"

namespace f110 {

// ------------------------------------------------------------------------
// k_agents: one thread per car.
// Heavy-first ray dispatch: the (car, chunk) waves whose longest ray took at
// least heavy_T lookups in the previous ray launch are listed (up to
// heavy_cap) for the leading blocks of this step's chunked ray kernel, so the
// rare long waves (grazing beams, up to ~400 lookups) start first instead of
// extending the launch's tail.  One atomic per wave of cars.
__device__ __forceinline__ void build_heavy_list(const StepArgs &a, int g, bool valid) {
    uint32_t hm = 0;
    int h = 0;
    if (valid) {
        const uint8_t *wc = a.wcost + (size_t)g * a.ray_nch;
        for (int k = 0; k < a.ray_nch; ++k)
            if (wc[k] >= a.heavy_T) {
                hm |= 1u << k;
                ++h;
            }
    }
    const int lane = threadIdx.x & 63;
    int incl = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const int total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total > 0) base = atomicAdd(a.heavy_count + a.parity, (uint32_t)total);
    base = __shfl(base, 63, 64);
    uint32_t pos = base + (uint32_t)(incl - h), keep = 0;
    uint32_t *list = a.heavy_list + (size_t)a.parity * a.heavy_cap;
    for (uint32_t m = hm; m; m &= m - 1) {
        const int k = __builtin_ctz(m);
        if (pos < (uint32_t)a.heavy_cap) {
            list[pos] = ((uint32_t)g << 8) | (uint32_t)k;
            keep |= 1u << k;
        }
        ++pos;
    }
    if (valid) a.heavy_mask[g] = keep;
}

__device__ __forceinline__ float bearing_f32(float y, float x) {  // atan2(y, x) within ~2e-4 rad (finite x, y)
    const float ax = fabsf(x), ay = fabsf(y);
    const float a = __fdividef(fminf(ax, ay), fmaxf(ax, ay));
    const float s = a * a;
    float r = ((-0.0464964749f * s + 0.15931422f) * s - 0.327622764f) * s * a + a;
    if (ay > ax) r = 1.57079637f - r;
    if (x < 0.0f) r = 3.14159274f - r;
    if (y < 0.0f) r = -r;
    return (ax == 0.0f && ay == 0.0f) ? 0.0f : r;
}

// The 64-beam chunks of car g whose f64 scans k_post_multi may read (bit k: chunk k), for the ray
// kernel's hand-off: its agent ray_cast visits only beams of each (car, opponent) pair's blocked
// view [lo, hi] -- the nearest beams of the opponent box's vertex bearings
// (get_blocked_view_indices, laser_models.py:282-315) -- seen from the car's yaw or, after a TTC
// response, from yaw 0 (base_classes.py:246-249).  Here in f32 (the box from fast sin / cos, the
// bearings from a polynomial atan2 good to ~2e-4 rad: errors far below a beam's 4.4e-3 rad for
// vertices beyond the 1 cm cutoff while |x|, |y| < 1 km (f32 position rounding ulp(coord) / 1 cm
// stays under a beam there; f110_create keeps no mask for a map that reaches beyond), the
// range widened by 3 beams; a bearing within 1e-2 rad of the +-pi wrap, a vertex within 1 cm of the
// car, or a NaN, marks every chunk.  The other chunks skip the hand-off store (its stores cost the
// two-agent ray launch ~6 %).  The poses of an env's cars meet in LDS: A divides 64 (the context
// allocates no mask otherwise).
// sx / sy / sth: the block's cars' poses (LDS, k_agents writes them before a barrier).
__device__ void handoff_chunks(const StepArgs &a, int g, const float *sx, const float *sy, const float *sth,
                               float len, float wid) {
    const int t = (int)threadIdx.x;
    const int A = a.A, B = a.B;
    const int ag = g % A, t0 = t - ag;  // the env's first car in the block
    const int nch = (B + 63) >> 6;
    const uint32_t all = nch >= 32 ? 0xFFFFFFFFu : ((1u << nch) - 1u);
    const float half_fov = (float)(a.fov * 0.5), inv_incr = (float)(1.0 / a.beam_incr);
    const float xi = sx[t], yi = sy[t];
    uint32_t m = nch > 32 ? all : 0u;
    for (int j = 0; j < A && m != all; ++j) {
        if (j == ag) continue;
        float sj, cj;
        __sincosf(sth[t0 + j], &sj, &cj);
        const float px[4] = {-len / 2, -len / 2, len / 2, len / 2};
        const float py[4] = {wid / 2, -wid / 2, -wid / 2, wid / 2};
        float bear[4];
        bool unsure = !(sth[t] == sth[t]);
        for (int q = 0; q < 4; ++q) {
            const float vx = cj * px[q] - sj * py[q] + sx[t0 + j], vy = sj * px[q] + cj * py[q] + sy[t0 + j];
            const float dx = vx - xi, dy = vy - yi;
            // NaN / inf, or a vertex within 1 cm of the car (its f32 bearing is not reliable there; the
            // reference's is NaN at distance 0: beam 0)
            unsure |= !(dx == dx) || !(dy == dy) || fabsf(dx) > 1e30f || fabsf(dy) > 1e30f ||
                      fabsf(dx) + fabsf(dy) < 0.01f;
            bear[q] = bearing_f32(dy, dx);
        }
        for (int w = 0; w < 2 && !unsure; ++w) {
            const float ego = w == 0 ? sth[t] : 0.0f;
            int lo = B, hi = -1;
            for (int q = 0; q < 4; ++q) {
                float ang = ego - bear[q];
                unsure |= !(fabsf(fabsf(ang) - 3.14159265f) > 1e-2f);
                if (ang > 3.14159265f) ang -= 6.28318531f;
                else if (ang < -3.14159265f) ang += 6.28318531f;
                const float gk = (half_fov - ang) * inv_incr;
                const int k = gk < 0.0f ? 0 : (gk > (float)(B - 1) ? B - 1 : (int)(gk + 0.5f));
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
            }
            lo = lo - 3 < 0 ? 0 : lo - 3;
            hi = hi + 3 > B - 1 ? B - 1 : hi + 3;
            m |= (2u << (hi >> 6)) - (1u << (lo >> 6));  // chunks lo / 64 .. hi / 64 (hi / 64 <= 31)
        }
        if (unsure) m = all;
    }
    a.hmask[g] = (a.hcheck & 4) ? 0u : m;  // f110_debug_set_handoff_check bit 2: a forced miss
}

// HMASK: the context keeps hand-off chunk masks (A >= 2 dividing 64): the block's new poses meet in
// LDS after the update and each car's mask is written at the end; without it the update's stores
// follow it directly (the single-agent form, one dependent chain less to schedule around a barrier).
// PENV: the context holds a per-car table of the dynamics fields (a.ptab, f110_set_env_params): the
// car's row is loaded with the prologue and update_pose reads a local f110_params built from it
// (width, length, lidar_max from a.pa[ag]); with a range table too (a.prange) a resetting car first
// redraws its row (param_draw) and stores it.  Without PENV nothing of this is compiled in.
// SPAWN: the context draws start states (a.srange, f110_set_spawn_randomization): the agent's range
// block is loaded with the prologue, and a resetting car perturbs its base pose (f110_spawn.h: the
// gap's table row, the cleared lateral offset, the heading offset), starts at the drawn speed and
// stores (x, y, yaw, speed) in a.spawn_state.  Without SPAWN nothing of this is compiled in.
template <bool HMASK, bool PENV, bool SPAWN>
__global__ void __launch_bounds__(64) k_agents(StepArgs a) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    const int EA = a.E * a.A;
    const bool valid = g < EA;
    const int A = a.A;
    const int e = valid ? g / A : 0;
    const int ag = valid ? g - e * A : 0;  // padding threads: agent 0 (a.pa holds A entries)
    // Every input of the car is loaded first, before the heavy-list atomic
    // and before anything waits: one memory round trip for the whole prologue.
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double b0 = 0.0, b1 = 0.0, raw_steer = 0.0, vel = 0.0;
    int cnt = 0, gate = 0;
    uint32_t episode = 0;
    uint64_t nstep = 0;
    double pv[PENV ? kDynFields : 1] = {};  // the car's table row (padding threads read none)
    f110_spawn_range sr = {};                // the agent's spawn ranges
    if (valid) {
        if (SPAWN) sr = a.srange[ag];
        if (ag == 0) nstep = a.nstep[e];
        if (PENV) {
#pragma unroll
            for (int k = 0; k < kDynFields; ++k) pv[k] = a.ptab[(size_t)k * EA + g];
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] = a.st[(size_t)k * EA + g];
        b0 = a.sb[g];
        b1 = a.sb[EA + g];
        cnt = a.scnt[g];
        if (a.mode == 1) {
            gate = a.reset_mask ? a.reset_mask[e] : 1;
        } else {
            gate = a.autoreset ? a.pending[e] : 0;
            episode = a.episode[e];
            if (a.actions_f64) {
                raw_steer = a.actions_f64[(size_t)g * 2];
                vel = a.actions_f64[(size_t)g * 2 + 1];
            } else {
                raw_steer = (double)a.actions[(size_t)g * 2];
                vel = (double)a.actions[(size_t)g * 2 + 1];
            }
        }
    }
    // RaceCar ag's box (its opponents' vertices for the hand-off mask), loaded with the prologue
    const float box_len = HMASK ? (float)a.pa[ag].length : 0.0f, box_wid = HMASK ? (float)a.pa[ag].width : 0.0f;
    if (a.heavy_build) build_heavy_list(a, g, valid);  // block-uniform branch, before any return
    // an LDS copy of cr_sincos's table (sin / cos of i/64): every sincos of the car's update reads it
    // there (a short dependent load instead of a trip to L1 / L2); the loads go out with the prologue's
    __shared__ double sct[256];  // F110_SINCOS_TAB_N x 4 doubles, padded to 4 per thread
    {
        static_assert(F110_SINCOS_TAB_N * 4 <= 256, "the LDS copy holds the table");
        constexpr int NT = F110_SINCOS_TAB_N * 4;
        const double *src = &kSinCosTab[0][0];
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = (int)threadIdx.x + 64 * i;
            v[i] = src[k < NT ? k : NT - 1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) sct[threadIdx.x + 64 * i] = v[i];
        __syncthreads();
    }
    const double(*tab)[4] = reinterpret_cast<const double(*)[4]>(sct);
#ifdef F110_AGENTS_PHASES  // timing build (scripts/agents_phases.py): counters 8-12 = s_memrealtime ticks per phase
    // and wave, summed (prologue + reset, update_pose, scan pose + first lookup, beam runs: 8-11), 13 = waves
    uint64_t tph = __builtin_amdgcn_s_memrealtime();
    auto aphase = [&](int k) {
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t t = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0)
            atomicAdd(a.ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride + 8 + k, (unsigned long long)(t - tph));
        tph = t;
        __builtin_amdgcn_sched_barrier(0);
    };
#else
    auto aphase = [](int) {};
#endif
    // the car's update (its returns leave the lambda: the hand-off poses below need every thread)
    int do_reset = 0;
    bool act = false;
    // the update's stores, the scan pose, the first lookup and the beam runs
    auto tail = [&]() {
#pragma unroll
    for (int k = 0; k < 7; ++k) a.st[(size_t)k * EA + g] = s[k];
    a.sb[g] = b0;
    a.sb[EA + g] = b1;
    a.scnt[g] = cnt;
    // scan pose (base_classes.py:420-422) and everything every ray of this car shares
    // base_classes.py:420-422; with lidar_dist == 0 the offset is +-0 for any
    // finite yaw, so the transcendentals are skipped (a non-finite yaw keeps
    // the reference's NaN)
    const bool no_offset = a.lidar_dist == 0.0 && isfinite(s[4]);
    double sy4 = 0.0, cy4 = 1.0;
    if (!no_offset) cr_sincos(s[4], sy4, cy4, tab);
    const double sx = no_offset ? s[0] + 0.0 : s[0] + a.lidar_dist * cy4;
    const double sy = no_offset ? s[1] + 0.0 : s[1] + a.lidar_dist * sy4;
    a.ray0[g] = sx;
    a.ray0[EA + g] = sy;
    a.ray0[2 * EA + g] = a.map.dt[cell_index(a.map, sx, sy)];  // first lookup (laser_models.py:129)
    aphase(2);
    double t0 = first_theta_index(s[4], a.fov, a.theta_dis);
    a.nruns[g] = build_beam_runs_fast(t0, a.inc, a.theta_dis, a.B, a.runs + (size_t)g * kMaxSeg, kMaxSeg);
    aphase(3);
    a.ttc_hit[g] = 0;
    if (ag == 0) {
        a.reset_flag[e] = (uint8_t)do_reset;
        a.noise_step[e] = do_reset ? 0ull : nstep;
    }
    };
    auto car = [&]() {
    if (!valid) return;
    const uint64_t genv = (uint64_t)(a.env_offset + e);
    if (a.mode == 1) {
        if (!gate) return;
        do_reset = 1;
    } else {
        do_reset = gate ? 1 : 0;
    }
    if (do_reset) {
        // RaceCar.reset (base_classes.py:183-204), then F110Env.reset's zero-action step (f110_env.py:457)
        const double *pz;
        SpawnDraws sw = {};
        if (SPAWN) sw = spawn_draws(a.sseed, genv, ag, a.mode == 1 ? 0ull : (uint64_t)episode + 1ull, sr);
        if (a.mode == 1) {
            pz = a.reset_poses + (size_t)g * 3;
        } else {
            uint32_t k = spawn_draw(a.seed, genv, episode) % (uint32_t)a.n_spawn;
            int col = ag;
            if (SPAWN && !spawn_own_column(sr)) {  // the gap: column 0 of the shifted row
                k = spawn_shift_row(k, sw.mag, sw.behind, (uint32_t)a.n_spawn);
                col = 0;
            }
            pz = a.spawn + ((size_t)k * A + col) * 3;
        }
        // float32 options (train_ddpg's dtype): the poses are float32 values
        // and start_rot is NumPy's float32 cos / sin of the float32 yaw
        double px = pz[0], py = pz[1], pth = pz[2];
        double ss[4] = {0.0, 0.0, 0.0, 0.0};
        if (SPAWN) {  // the perturbed pose, rounded under float32 options where the base pose is
            spawn_pose(a.map, px, py, pth, sw, sr.clearance, a.reset_f32 != 0, ss, tab);
            px = ss[0];
            py = ss[1];
            pth = ss[2];
        } else if (a.reset_f32) {
            px = (double)(float)px;
            py = (double)(float)py;
            pth = (double)(float)pth;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] = 0.0;
        s[0] = px;
        s[1] = py;
        s[4] = pth;
        if (SPAWN) {
            s[3] = ss[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) a.spawn_state[(size_t)k * EA + g] = ss[k];
        }
        b0 = b1 = 0.0;
        cnt = 0;
        raw_steer = 0.0;
        vel = 0.0;
        a.start[g] = px;
        a.start[EA + g] = py;
        a.start[2 * EA + g] = pth;
        if (ag == a.ego) {  // F110Env.reset's start_rot (f110_env.py:448-451), once per episode
            if (a.reset_f32) {
                const float nt = -(float)pth;
                a.start_rot[e] = (double)np_sincosf(nt, true);
                a.start_rot[a.E + e] = (double)np_sincosf(nt, false);
            } else {
                double sr, crr;
                cr_sincos(-pth, sr, crr, tab);
                a.start_rot[e] = crr;
                a.start_rot[a.E + e] = sr;
            }
        }
        a.toggles[g] = 0;
        a.near_start[g] = 1;
        a.lap_times[g] = 0.0f;
        a.lap_counts[g] = 0.0f;
        if (PENV && a.prange) {  // domain randomization: this episode's car, in force from the reset's own step
            param_draw(a.pseed, genv, ag, a.mode == 1 ? 0ull : (uint64_t)episode + 1ull,
                       a.prange + (size_t)ag * 2 * kDynFields, pv);
#pragma unroll
            for (int k = 0; k < kDynFields; ++k) a.ptab[(size_t)k * EA + g] = pv[k];
        }
    }
    aphase(0);
    if (PENV) {
        f110_params lp = a.pa[ag];  // width, length, lidar_max stay the agent's
        __builtin_memcpy(&lp, pv, kDynFields * sizeof(double));  // the leading doubles (f110_env_rows.h)
        update_pose(s, b0, b1, cnt, raw_steer, vel, lp, a.dt, a.integrator, tab);
    } else {
        update_pose(s, b0, b1, cnt, raw_steer, vel, a.pa[ag], a.dt, a.integrator, tab);  // RaceCar.params (per agent)
    }
    aphase(1);
    act = true;
    if (!HMASK) tail();
    };
    car();
#ifdef F110_AGENTS_PHASES
    if ((threadIdx.x & 63) == 0) atomicAdd(a.ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride + 13, 1ull);
#endif
    if (HMASK) {
        // the hand-off mask's poses (every car of the block, the new or the unchanged ones), shared
        // before the state stores so that the barrier waits on no memory operation
        __shared__ float hx[64], hy[64], hth[64];
        hx[threadIdx.x] = (float)s[0];
        hy[threadIdx.x] = (float)s[1];
        hth[threadIdx.x] = (float)s[4];
        __syncthreads();
        if (valid) handoff_chunks(a, g, hx, hy, hth, box_len, box_wid);  // (A divides 64: an env's cars share the block)
        if (act) tail();
    }
}

// 64-thread blocks: a few thousand cars must still spread over all CUs.  <HMASK, PENV, SPAWN>: a context
// without hand-off masks / a per-env table / spawn ranges launches the instantiations compiled without them.
hipError_t launch_agents(const StepArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    static void (*const fn[2][2][2])(StepArgs) = {
        {{k_agents<false, false, false>, k_agents<false, false, true>},
         {k_agents<false, true, false>, k_agents<false, true, true>}},
        {{k_agents<true, false, false>, k_agents<true, false, true>},
         {k_agents<true, true, false>, k_agents<true, true, true>}}};
    const int EA = a.E * a.A;
    hipExtLaunchKernelGGL(fn[a.hmask != nullptr][a.ptab != nullptr][a.srange != nullptr], dim3((EA + 63) / 64), dim3(64),
                          0, s, start, stop, 0, a);
    return hipGetLastError();
}

}  // namespace f110
