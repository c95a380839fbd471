// f110_post.hip — the post stage of an env step (f110_step.cpp), after the ray kernel: one thread
// per env (k_post_single) or two waves per env (k_post_multi: GJK, agent ray_cast): TTC response,
// obs packing, _check_done and the env's episode bookkeeping.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "../../include/f110.h"
#include "f110_env_rows.h"
#include "f110_geometry.h"
#include "f110_math.h"
#include "f110_sincos.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

// F110Env.step's time + _check_done (f110_env.py:404-406, :310-352) and the
// env's autoreset / episode / noise bookkeeping, for env e.  Split in two so
// the kernels issue every load of it at their start, together with their own
// loads: one memory round trip instead of a chain of dependent ones (the
// stores in between would otherwise keep the compiler from hoisting them).
struct EpiCar {  // per car: lap bookkeeping
    double sx, sy;
    int32_t tg;
    float lt;
    uint32_t ns;
};
struct EpiEnv {  // per env
    double tprev, ct, st;
    uint64_t nstep;
    uint32_t episode;
    int32_t stall;  // the stall counter (f110_set_episode_limits with a stall limit; else unused)
};

// LIM (the post kernels, their epilogue and its loads): an episode limit is on
// (f110_set_episode_limits).  Without it nothing of the limits is compiled in: a context with both
// limits 0 launches the limit-free instantiations, the kernels from before there were limits.

__device__ __forceinline__ void epilogue_load_car(const StepArgs &a, int g, EpiCar &c) {
    const int EA = a.E * a.A;
    c.sx = a.start[g];
    c.sy = a.start[EA + g];
    c.tg = a.toggles[g];
    c.ns = a.near_start[g];
    c.lt = a.lap_times[g];
}

template <bool LIM>
__device__ __forceinline__ void epilogue_load_env(const StepArgs &a, int e, EpiEnv &v) {
    v.tprev = a.sim_time[e];
    v.ct = a.start_rot[e];  // cos(-th), sin(-th) of the ego start yaw
    v.st = a.start_rot[a.E + e];
    v.nstep = a.noise_step[e];  // written by this step's k_agents
    const uint32_t ep = a.episode[e];  // (loaded whatever the mode: one round trip with the others)
    v.episode = a.mode == 0 ? ep : 0u;
    v.stall = (LIM && a.stall_steps) ? a.stall[e] : 0;  // with the others: no dependent round trip
}

// stl: post-TTC state rows of its A agents (x at [i*stride], y at
// [i*stride + 1]); col: collision flags; cars / env: the prefetched inputs;
// vego: the ego's post-TTC state[3] (read only under a stall limit).
template <bool LIM>
__device__ void env_epilogue(const StepArgs &a, int e, const double *stl, int stride, const int32_t *col,
                             int do_reset, const EpiEnv &v, const EpiCar *cars, double vego) {
    const int A = a.A;
    const double tnow = (do_reset ? 0.0 : v.tprev) + a.dt;
    a.sim_time[e] = tnow;
    const double r00 = v.ct, r01 = -v.st, r10 = v.st, r11 = v.ct;
    bool all4 = true;
    for (int i = 0; i < A; ++i) {
        const int g = e * A + i;
        const EpiCar &c = cars[i];
        double px = stl[i * stride] - c.sx;
        double py = stl[i * stride + 1] - c.sy;
        // np.dot(start_rot, [dx; dy]) (f110_env.py:330) is a BLAS dgemm: on
        // the reference's host each row is fma(r_i1, py, r_i0 * px)
        // (measured, tests/golden/env_lap_f32.npz; the float32 start_rot is
        // widened to f64 first)
        double dx = fma(r01, py, r00 * px);
        double dy = fma(r11, py, r10 * px);
        double ty;
        if (dy > 2.0) ty = dy - 2.0;
        else if (dy < -2.0) ty = -2.0 - dy;
        else ty = 0.0;
        bool close = dx * dx + ty * ty <= 0.1;
        int tg = c.tg;
        uint32_t ns = c.ns;
        if (close && !ns) { ns = 1; ++tg; }
        else if (!close && ns) { ns = 0; ++tg; }
        a.toggles[g] = tg;
        a.near_start[g] = (uint8_t)ns;
        float lc = (float)(tg / 2);
        float lt = tg < 4 ? (float)tnow : c.lt;
        a.lap_counts[g] = lc;
        a.lap_times[g] = lt;
        if (a.out.lap_counts) a.out.lap_counts[g] = lc;
        if (a.out.lap_times) a.out.lap_times[g] = lt;
        all4 = all4 && tg >= 4;
    }
    bool term = col[a.ego] || all4;
    if (a.out.terminated) a.out.terminated[e] = term ? 1 : 0;
    if (a.out.was_reset) a.out.was_reset[e] = (uint8_t)do_reset;
    if (a.out.sim_time) a.out.sim_time[e] = tnow;
    // episode limits (f110_set_episode_limits): n = v.nstep, this step's noise counter, is the steps
    // since the env's reset on every path (0 in the reset's own step: k_agents, f110_reset's masked
    // envs and autoresets alike; + 1 per step below; an unmasked env of a masked reset is not here)
    bool trunc = false;
    if (LIM) {
        int32_t s = 0;
        if (a.stall_steps) {
            // (saturating: without autoreset a standing env counts on for as long as it is stepped)
            s = do_reset ? 0 : (fabs(vego) < a.stall_speed ? (v.stall < INT32_MAX ? v.stall + 1 : v.stall) : 0);
            a.stall[e] = s;
        }
        const uint8_t code = (term || do_reset) ? (uint8_t)0 : truncation_code(v.nstep, s, a.max_steps, a.stall_steps);
        if (a.truncated) a.truncated[e] = code;
        trunc = code != 0;
    }
    a.pending[e] = (a.autoreset && (term || trunc)) ? 1 : 0;
    // autoreset spawn draws count episodes from the env's last explicit reset, so a
    // reset replays the same trajectory whatever ran before it (the bench's
    // trajectory digest compares N = 1 and N > 1 runs after a clock ramp)
    const uint32_t ep = do_reset ? (a.mode == 0 ? v.episode + 1 : 0u) : v.episode;
    if (do_reset) a.episode[e] = ep;
    a.nstep[e] = v.nstep + 1;
}

// k_post_single: single-agent envs after the FUSED ray kernel, one thread per
// env: the TTC response (RaceCar.check_ttc, base_classes.py:246-249), the
// pose part of the observation, collisions and the env epilogue.
template <bool LIM>
__global__ void __launch_bounds__(64) k_post_single(StepArgs a) {
    reset_next_heavy(a);
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.E) return;
    if (a.mode == 1 && a.reset_mask && !a.reset_mask[e]) return;
    const int EA = a.E;  // A == 1: car g == env e
    // every input first (one memory round trip), then the stores
    double stl[2] = {a.st[e], a.st[EA + e]};
    double yaw = a.st[(size_t)4 * EA + e];
    int32_t col = a.ttc_hit[e];
    const int do_reset = a.reset_flag[e];
    const double vego = (LIM && a.stall_steps) ? a.st[(size_t)3 * EA + e] : 0.0;  // (a stall limit only)
    EpiCar car;
    EpiEnv env;
    epilogue_load_car(a, e, car);
    epilogue_load_env<LIM>(a, e, env);
    if (col) {  // state[3:] = 0 (yaw included)
#pragma unroll
        for (int k = 3; k < 7; ++k) a.st[(size_t)k * EA + e] = 0.0;
        yaw = 0.0;
    }
    if (a.out.obs) {
        float *o = a.out.obs + (size_t)e * obs_row(a) + a.B;
        const float4 v = make_float4((float)stl[0], (float)stl[1], (float)wrap_angle(yaw), col ? 1.0f : 0.0f);
        if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {  // one 16-byte store (the default obs row is aligned)
            *reinterpret_cast<float4 *>(o) = v;
        } else {
            o[0] = v.x;
            o[1] = v.y;
            o[2] = v.z;
            o[3] = v.w;
        }
    }
    if (a.out.collisions) a.out.collisions[e] = (uint8_t)col;
    env_epilogue<LIM>(a, e, stl, 2, &col, do_reset, env, &car, col ? 0.0 : vego);
}

// LDS hand-off between the lanes of ONE wave (no workgroup barrier).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// k_post_multi: multi-agent envs after the tiled ray kernel (TTC flags are
// already set).  Two waves per env and no LDS copy of the scans: the agent
// ray_cast edits the f64 hand-off in place, so many envs stay resident per CU
// and their serial phases overlap.  Wave 0 runs GJK (collision_multiple on
// the pre-TTC poses) while wave 1 builds each (car, opponent) pair's box,
// blocked beam range and beam window (on the post-TTC pose).
constexpr int kMultiBlock = 128;  // one wave per env measured no faster (0.398 vs 0.392 ms per C4 step)

struct MultiShared {
    double stl[kMaxAgents][7];   // state after the TTC response
    double pose0[kMaxAgents][3]; // agent_poses: before the TTC response (base_classes.py:587)
    double verts[kMaxAgents][8]; // Simulator.check_collision's boxes (Simulator.params)
    double rv[kMaxAgents * (kMaxAgents - 1)][8];  // opponent j seen by car i (RaceCar i's params)
    double wcen[kMaxAgents * (kMaxAgents - 1)], whalf[kMaxAgents * (kMaxAgents - 1)];
    double phi[kMaxAgents * (kMaxAgents - 1)][4];  // vertex bearings of each pair's box
    double ego[kMaxAgents];                        // atan2(sin(yaw), cos(yaw)), post-TTC
    int32_t kq[kMaxAgents * (kMaxAgents - 1)][4];  // nearest beam of each vertex
    int32_t blo[kMaxAgents * (kMaxAgents - 1)], bhi[kMaxAgents * (kMaxAgents - 1)];
    int32_t rng[kMaxAgents * (kMaxAgents - 1)][4]; // window_beam_ranges, clipped to [blo, bhi]
    int32_t col[kMaxAgents];
    int32_t ttc[kMaxAgents];  // the car's TTC fired (its state[3:] was zeroed)
    EpiCar epi[kMaxAgents];  // env_epilogue inputs, prefetched at kernel start
    EpiEnv epe;
    int32_t do_reset;
};

// beams of pair pr's ray_cast pass (window_beam_ranges clipped to lo..hi)
__device__ __forceinline__ int pass_beams(const MultiShared &sh, int pr) {
    const int n0 = sh.rng[pr][1] - sh.rng[pr][0] + 1;
    const int n1 = sh.rng[pr][3] - sh.rng[pr][2] + 1;
    return (n0 > 0 ? n0 : 0) + (n1 > 0 ? n1 : 0);
}


template <bool LIM>
__global__ void __launch_bounds__(kMultiBlock, 6) k_post_multi(StepArgs a) {
    reset_next_heavy(a);
    __shared__ MultiShared sh;
    const int e = blockIdx.x;
    const int tid = threadIdx.x;
    const int A = a.A, B = a.B;
    const int EA = a.E * A;
    if (a.mode == 1 && a.reset_mask && !a.reset_mask[e]) return;  // uniform per block
#ifdef F110_POST_PHASES  // timing build (scripts/post_phases.py): counters 8-11 = wall_clock64 ticks per phase, 12 = blocks
    uint64_t tph = wall_clock64();
    auto phase = [&](int k) {
        const uint64_t t = wall_clock64();
        if (tid == 0) atomicAdd(a.ctr + (size_t)(e % kCtrSlots) * kCtrStride + 8 + k, (unsigned long long)(t - tph));
        tph = t;
    };
#else
    auto phase = [](int) {};
#endif
    double *scan = a.scan + (size_t)e * A * B;
    if (tid < A) {
        const int g = e * A + tid;
#pragma unroll
        for (int k = 0; k < 7; ++k) sh.stl[tid][k] = a.st[(size_t)k * EA + g];
        sh.pose0[tid][0] = sh.stl[tid][0];
        sh.pose0[tid][1] = sh.stl[tid][1];
        sh.pose0[tid][2] = sh.stl[tid][4];
        epilogue_load_car(a, g, sh.epi[tid]);
        get_vertices(sh.stl[tid][0], sh.stl[tid][1], sh.stl[tid][4], a.p.length, a.p.width, sh.verts[tid]);
        const int hit = a.ttc_hit[g];
        sh.col[tid] = hit;  // Simulator.step :601-602
        sh.ttc[tid] = hit;
        if (hit) {          // RaceCar.check_ttc (base_classes.py:246-249): state[3:] = 0
#pragma unroll
            for (int k = 3; k < 7; ++k) {
                sh.stl[tid][k] = 0.0;
                a.st[(size_t)k * EA + g] = 0.0;
            }
        }
    }
    if (tid == 0) {
        sh.do_reset = a.reset_flag[e];
        epilogue_load_env<LIM>(a, e, sh.epe);
    }
    __syncthreads();
    phase(0);
    if (tid == 0) {  // collision_multiple (collision_models.py:184-212)
        for (int i = 0; i < A - 1; ++i)
            for (int j = i + 1; j < A; ++j)
                if (gjk_collision(sh.verts[i], sh.verts[j])) {
                    sh.col[i] = 1;
                    sh.col[j] = 1;
                }
    }
    if (tid >= 64 && a.geo_ready) {
        // the ray launch's geometry blocks computed every pair from the pre-TTC poses; a car whose
        // TTC fired sees its opponents from a zeroed yaw: its pairs are recomputed here
        const int lane = tid & 63;
        const int NP = A * (A - 1);
        for (int pr = lane; pr < NP; pr += 64) {
            const int i = pr / (A - 1);
            const int jj = pr - i * (A - 1);
            const int j = jj < i ? jj : jj + 1;
            if (sh.ttc[i]) {
                pair_geometry_ool(sh.stl[i][0], sh.stl[i][1], sh.stl[i][4], sh.pose0[j][0], sh.pose0[j][1],
                                  sh.pose0[j][2], a.pa[i].length, a.pa[i].width, B, a.fov, a.beam_incr, sh.rv[pr],
                                  sh.phi[pr], &sh.wcen[pr], &sh.whalf[pr], sh.rng[pr]);
            } else {
                const PairGeom &o = a.geo[(size_t)e * NP + pr];
#pragma unroll
                for (int k = 0; k < 8; ++k) sh.rv[pr][k] = o.rv[k];
                sh.wcen[pr] = o.wc;
                sh.whalf[pr] = o.wh;
#pragma unroll
                for (int k = 0; k < 4; ++k) sh.rng[pr][k] = o.rng[k];
            }
        }
    } else if (tid >= 64) {
        // per-pair geometry (on wave 1 when there are two), spread over lanes:
        // boxes and ego headings, then one (pair, vertex) per lane, then
        // per-pair reductions
        const int lane = tid & 63;
        const int NP = A * (A - 1);
        for (int pr = lane; pr < NP; pr += 64) {
            const int i = pr / (A - 1);
            const int jj = pr - i * (A - 1);
            const int j = jj < i ? jj : jj + 1;
            // RaceCar.ray_cast_agents: get_vertices(opp_pose, self.params['length'], self.params['width'])
            const f110_params &pi = a.pa[i];
            get_vertices(sh.pose0[j][0], sh.pose0[j][1], sh.pose0[j][2], pi.length, pi.width, sh.rv[pr]);
        }
        if (lane < A) {  // atan2(sin, cos) of the post-TTC yaw
            double ys, yc;
            cr_sincos(sh.stl[lane][4], ys, yc);
            sh.ego[lane] = atan2(ys, yc);
        }
        wave_sync();
        for (int w = lane; w < 4 * NP; w += 64) {  // get_blocked_view_indices, one vertex per lane
            const int pr = w >> 2, q = w & 3;
            const int i = pr / (A - 1);
            sh.kq[pr][q] = blocked_vertex_beam(sh.stl[i][0], sh.stl[i][1], sh.ego[i], sh.rv[pr][2 * q],
                                               sh.rv[pr][2 * q + 1], B, a.fov, a.beam_incr, sh.phi[pr][q]);
        }
        wave_sync();
        for (int pr = lane; pr < NP; pr += 64) {
            const int i = pr / (A - 1);
            int lo = sh.kq[pr][0], hi = sh.kq[pr][0];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                lo = sh.kq[pr][q] < lo ? sh.kq[pr][q] : lo;
                hi = sh.kq[pr][q] > hi ? sh.kq[pr][q] : hi;
            }
            sh.blo[pr] = lo;
            sh.bhi[pr] = hi;
            double wc, wh;
            box_beam_window(sh.stl[i][0], sh.stl[i][1], sh.rv[pr], sh.phi[pr], wc, wh);
            sh.wcen[pr] = wc;
            sh.whalf[pr] = wh;
            int r0a, r0b, r1a, r1b;
            window_beam_ranges(sh.stl[i][4], a.fov, a.beam_incr, B, wc, wh, r0a, r0b, r1a, r1b);
            sh.rng[pr][0] = r0a > lo ? r0a : lo;  // beams lo..hi of ray_cast's loop that the window can hold
            sh.rng[pr][1] = r0b < hi ? r0b : hi;
            sh.rng[pr][2] = r1a > lo ? r1a : lo;
            sh.rng[pr][3] = r1b < hi ? r1b : hi;
        }
    }
    __syncthreads();
    phase(1);
    // agent ray_cast (base_classes.py:206-227; laser_models.py:318-346), one
    // opponent at a time per car (each pass min-updates the same beams), all
    // cars' passes of one round in one sweep over the block; only the beams
    // of lo..hi that the box's window can hold are visited
    for (int jj = 0; jj < A - 1; ++jj) {
        int total = 0;
        for (int i = 0; i < A; ++i) total += pass_beams(sh, i * (A - 1) + jj);
        for (int item = tid; item < total; item += kMultiBlock) {
            int i = 0, k = item;
            for (int n = pass_beams(sh, jj); k >= n; n = pass_beams(sh, i * (A - 1) + jj)) {
                k -= n;
                ++i;
            }
            const int pr = i * (A - 1) + jj;
            const int n0 = sh.rng[pr][1] - sh.rng[pr][0] + 1;
            const int b = k < (n0 > 0 ? n0 : 0) ? sh.rng[pr][0] + k : sh.rng[pr][2] + k - (n0 > 0 ? n0 : 0);
            const double ox = sh.stl[i][0], oy = sh.stl[i][1], oth = sh.stl[i][4];
            const double *v = sh.rv[pr];
            const double ang = beam_angle(b, a.fov, a.beam_incr);
            if (!(fabs(wrap_pm_pi(oth + ang - sh.wcen[pr])) <= sh.whalf[pr])) continue;  // box_beam_window
            if ((a.hcheck & 1) && a.hmask && !((a.hmask[(size_t)e * A + i] >> (b >> 6)) & 1u))  // debug: a hand-off miss
                atomicAdd(a.ctr + (size_t)(e % kCtrSlots) * kCtrStride + 6, 1ull);
            const double bt = oth + ang + kPi / 2.;
            double v31, v30;
            cr_sincos(bt, v31, v30);
            double cur = scan[i * B + b];
            const double cur0 = cur;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int q1 = (q + 1) & 3;
                const double rr = get_range(ox, oy, v30, v31, v[2 * q], v[2 * q + 1], v[2 * q1], v[2 * q1 + 1]);
                if (rr < cur) cur = rr;
            }
            if (cur != cur0) {  // patch the ray pass's outputs for this beam
                scan[i * B + b] = cur;
                const size_t o = ((size_t)e * A + i) * B + b;
                if (a.out.scans) a.out.scans[o] = (float)cur;
                if (a.out.scans_f64) a.out.scans_f64[o] = cur;
                if (i == 0 && a.out.obs) a.out.obs[(size_t)e * obs_row(a) + b] = obs_scan_value(cur, (float)a.p.lidar_max);
            }
        }
        __syncthreads();
    }
    phase(2);

    // ---- outputs --------------------------------------------------------
    // the scan entries were written by the ray pass (and patched above)
    if (a.out.obs && tid < A) {  // F110Env._pack_flat_obs, f110_env.py:552-584: pose entries
        float *o = a.out.obs + (size_t)e * obs_row(a) + B + 4 * tid;
        o[0] = (float)sh.stl[tid][0];
        o[1] = (float)sh.stl[tid][1];
        o[2] = (float)wrap_angle(sh.stl[tid][4]);
        o[3] = sh.col[tid] ? 1.0f : 0.0f;
    }
    if (a.out.collisions && tid < A) a.out.collisions[(size_t)e * A + tid] = (uint8_t)sh.col[tid];
    if (tid == 0) env_epilogue<LIM>(a, e, &sh.stl[0][0], 7, sh.col, sh.do_reset, sh.epe, sh.epi, LIM ? sh.stl[a.ego][3] : 0.0);
#ifdef F110_POST_PHASES
    phase(3);
    if (tid == 0) atomicAdd(a.ctr + (size_t)(e % kCtrSlots) * kCtrStride + 12, 1ull);
#endif
}

// k_post_single for single-agent envs (one thread per env), k_post_multi otherwise (one block per
// env), which reads the pair geometry of the ray launch when geo_ready.  <LIM>: an episode limit is
// on (f110_set_episode_limits).
hipError_t launch_post(const StepArgs &a, bool geo_ready, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    static void (*const fn[2][2])(StepArgs) = {{k_post_multi<false>, k_post_multi<true>},
                                               {k_post_single<false>, k_post_single<true>}};
    const bool single = a.A == 1, lim = a.max_steps != 0 || a.stall_steps != 0;
    StepArgs pa = a;
    if (!single) pa.geo_ready = geo_ready;
    hipExtLaunchKernelGGL(fn[single][lim], single ? dim3((a.E + 63) / 64) : dim3(a.E), dim3(single ? 64 : kMultiBlock),
                          0, s, start, stop, 0, pa);
    return hipGetLastError();
}

}  // namespace f110
