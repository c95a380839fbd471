// f110_race.hip — per-episode race outcomes of an autoresetting batch (f110_race_stats,
// include/f110.h "race statistics"): progress along the centerline, lead over the opponent, passes,
// how the episode ended.  Context-free like f110_reward.hip and f110_episode.hip: it reads a step's
// observations and flags, whoever produced them.
//
//   k_race_project  one wave per env, four envs per 256-thread block: the ego's point on lanes
//                   0-31, the opponent's on 32-63, through project_xy (f110_track_device.h), so
//                   the two dependent load chains (grid bounds -> midpoints -> segment ends)
//                   overlap and every cross-lane step stays inside its half.  A half whose car is
//                   missing or not finite idles as a whole: no half is ever divided around a
//                   shuffle.  The first lane of each half writes its car's fields of the env's
//                   RaceProj (one writer per element).  No LDS, no barrier.
//   k_race          one thread per env: every input of the row first, then race_update (f110_race.h,
//                   shared with the host hook), the per-env outputs, and the block's partial of the
//                   envs that finish, reduced in LDS as a binary tree over the thread index;
//   k_race_finish   one block: the block partials in ascending block order, then into the totals.
//
// Three launches instead of a last-block ticket: the stream orders the stores before the next
// pass, no fence and no atomic.  No floating-point atomics anywhere: the same inputs give the same
// bits.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_race.h"
#include "f110_task_args.h"
#include "f110_track_device.h"

namespace f110 {

namespace {

__global__ void __launch_bounds__(64 * kRaceProjEnvs) k_race_project(RaceArgs a) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (kHalf - 1);
    const int car = lane >> 5;  // 0: the ego's half, 1: the opponent's
    const int64_t e = (int64_t)blockIdx.x * kRaceProjEnvs + (threadIdx.x >> 6);
    if (e >= a.E) return;  // the whole wave
    const float *base = car ? a.opp : a.ego;  // half-uniform
    double x = 0.0, y = 0.0;
    bool ok = base != nullptr;
    if (ok) {
        const float *p = base + e * a.stride;
        x = (double)p[0];
        y = (double)p[1];
        ok = isfinite(x) && isfinite(y);
    }
    Proj pj{0.0, 0.0, 0};
    if (ok) pj = project_xy(a.track, x, y, sub);  // all 32 lanes of the half, or none
    if (sub != 0) return;
    RaceProj *o = a.proj + e;
    if (car == 0) {
        o->s0 = pj.s;
        o->t0 = pj.t;
        o->ok0 = ok ? 1 : 0;
    } else {
        o->s1 = pj.s;
        o->ok1 = ok ? 1 : 0;
    }
}

__global__ void __launch_bounds__(kRaceBlock) k_race(RaceArgs a) {
    __shared__ RacePart sh[kRaceBlock];
    const int tid = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * kRaceBlock + tid;
    RacePart p = race_part_empty();
    if (e < a.E) {
        // every input first: one memory round trip
        f110_race_state st = a.state[e];
        const RaceProj pr = a.proj[e];
        const int has_opp = a.opp != nullptr;
        const float c0 = a.ego[e * a.stride + 3];
        const float c1 = has_opp ? a.opp[e * a.stride + 3] : 0.0f;
        const int term = a.terminated[e];
        const int trunc = a.truncated ? a.truncated[e] : 0;
        const int wr = a.was_reset[e];
        RaceRow r;
        r.s[0] = pr.s0;
        r.s[1] = pr.s1;
        r.t0 = pr.t0;
        r.ok[0] = pr.ok0;
        r.ok[1] = has_opp ? pr.ok1 : 0;
        r.col[0] = c0 != 0.0f;
        r.col[1] = c1 != 0.0f;
        r.term = term;
        r.trunc = trunc;
        r.was_reset = wr;
        r.has_opp = has_opp;
        const int res = race_update(a.p, a.track.closed, a.track.L, r, st);
        a.state[e] = st;
        a.result[e] = (uint8_t)res;
        const double lead = race_lead(st, has_opp);
        if (a.cur) {
            a.cur[2 * e] = st.prog[0];
            a.cur[2 * e + 1] = lead;
        }
        if (res) {
            if (a.last_progress) a.last_progress[e] = st.prog[0];
            if (a.last_lead) a.last_lead[e] = lead;
            if (a.last_length) a.last_length[e] = st.len;
        }
        p = race_part(res, st, has_opp);
    }
    sh[tid] = p;
    __syncthreads();
#pragma unroll
    for (int h = kRaceBlock / 2; h >= 1; h >>= 1) {
        if (tid < h) race_merge(sh[tid], sh[tid + h]);
        __syncthreads();
    }
    if (tid == 0) a.part[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(kRaceBlock) k_race_finish(RaceArgs a, int nb) {
    __shared__ RacePart sh[kRaceBlock];
    __shared__ double psum[kRaceBlock], lsum[kRaceBlock];
    const int tid = threadIdx.x;
    RacePart acc = race_part_empty();  // thread 0's
    for (int base = 0; base < nb; base += kRaceBlock) {
        const int m = nb - base < kRaceBlock ? nb - base : kRaceBlock;
        RacePart p = race_part_empty();
        if (tid < m) p = a.part[base + tid];  // the loads in parallel
        psum[tid] = p.prog_sum;
        lsum[tid] = p.lead_sum;
        p.prog_sum = p.lead_sum = 0.0;
        sh[tid] = p;
        __syncthreads();
        // the counts, min and max do not depend on the order: a tree; the two sums do: thread 0 adds
        // the partials in ascending block order (two chains of dependent adds, nothing else on them)
        double s = acc.prog_sum, l = acc.lead_sum;
        if (tid == 0)
            for (int i = 0; i < m; ++i) {
                s += psum[i];
                l += lsum[i];
            }
#pragma unroll
        for (int h = kRaceBlock / 2; h >= 1; h >>= 1) {
            if (tid < h) race_merge(sh[tid], sh[tid + h]);
            __syncthreads();
        }
        if (tid == 0) {
            acc.prog_sum = acc.lead_sum = 0.0;
            race_merge(acc, sh[0]);
            acc.prog_sum = s;
            acc.lead_sum = l;
        }
        __syncthreads();
    }
    if (tid == 0) {
        f110_race_totals t = *a.totals;
        race_totals_add(t, acc);
        *a.totals = t;
    }
}

}  // namespace

hipError_t launch_race_stats(const RaceArgs &a, hipStream_t s) {
    if (a.E <= 0) return hipSuccess;
    const int64_t nb = race_blocks(a.E);
    const int64_t pb = (a.E + kRaceProjEnvs - 1) / kRaceProjEnvs;
    if (pb > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_race_project, dim3((unsigned)pb), dim3(64 * kRaceProjEnvs), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_race, dim3((unsigned)nb), dim3(kRaceBlock), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_race_finish, dim3(1), dim3(kRaceBlock), 0, s, a, (int)nb);
    return hipGetLastError();
}

}  // namespace f110
