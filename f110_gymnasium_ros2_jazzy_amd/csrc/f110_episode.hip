// f110_episode.hip — episode return / length bookkeeping of an autoresetting batch
// (f110_episode_stats, include/f110.h).  Context-free like f110_reward.hip: it reads a step's
// rewards and flags, whoever produced them.
//
//   k_episode         one thread per env: episode_update (f110_env_rows.h, shared with the host hook),
//                     the per-env outputs, and the block's partial of the envs that finish, reduced
//                     in LDS as a binary tree over the thread index (a fixed order);
//   k_episode_finish  one block: the block partials in ascending block order, then into the totals.
//
// Two launches instead of a last-block ticket: the stream orders the partials' stores before the
// finishing pass, no fence and no atomic.  No floating-point atomics anywhere: the same inputs give
// the same bits.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_env_rows.h"
#include "f110_task_args.h"

namespace f110 {

namespace {

__global__ void __launch_bounds__(kEpisodeBlock) k_episode(EpisodeArgs a) {
    __shared__ EpisodePart sh[kEpisodeBlock];
    const int tid = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * kEpisodeBlock + tid;
    EpisodePart p = {0, 0, 0, 0, 0.0, 0.0, 0.0};
    if (e < a.E) {
        // every input first: one memory round trip
        f110_episode_state st = a.state[e];
        const double r = a.rewards[e];
        const int term = a.terminated[e];
        const int trunc = a.truncated ? a.truncated[e] : 0;
        const int wr = a.was_reset[e];
        const int code = episode_update(r, term, trunc, wr, st);
        a.state[e] = st;
        if (a.finished) a.finished[e] = code ? 1 : 0;
        if (code) {
            if (a.last_return) a.last_return[e] = st.ret;
            if (a.last_length) a.last_length[e] = st.len;
        }
        p = episode_part(code, st);
    }
    sh[tid] = p;
    __syncthreads();
#pragma unroll
    for (int h = kEpisodeBlock / 2; h >= 1; h >>= 1) {
        if (tid < h) episode_merge(sh[tid], sh[tid + h]);
        __syncthreads();
    }
    if (tid == 0) a.part[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(kEpisodeBlock) k_episode_finish(EpisodeArgs a, int nb) {
    __shared__ EpisodePart sh[kEpisodeBlock];
    __shared__ double psum[kEpisodeBlock];
    const int tid = threadIdx.x;
    EpisodePart acc = {0, 0, 0, 0, 0.0, 0.0, 0.0};  // thread 0's
    for (int base = 0; base < nb; base += kEpisodeBlock) {
        const int m = nb - base < kEpisodeBlock ? nb - base : kEpisodeBlock;
        EpisodePart p = {0, 0, 0, 0, 0.0, 0.0, 0.0};
        if (tid < m) p = a.part[base + tid];  // the loads in parallel
        psum[tid] = p.sum;
        p.sum = 0.0;
        sh[tid] = p;
        __syncthreads();
        // the counts, min and max do not depend on the order: a tree; the return sum does: thread 0
        // adds the partials in ascending block order (a chain of dependent adds, nothing else on it)
        double s = acc.sum;
        if (tid == 0)
            for (int i = 0; i < m; ++i) s += psum[i];
#pragma unroll
        for (int h = kEpisodeBlock / 2; h >= 1; h >>= 1) {
            if (tid < h) episode_merge(sh[tid], sh[tid + h]);
            __syncthreads();
        }
        if (tid == 0) {
            acc.sum = 0.0;
            episode_merge(acc, sh[0]);
            acc.sum = s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        f110_episode_totals t = *a.totals;
        episode_totals_add(t, acc);
        *a.totals = t;
    }
}

}  // namespace

hipError_t launch_episode_stats(const EpisodeArgs &a, hipStream_t s) {
    if (a.E <= 0) return hipSuccess;
    const int64_t nb = episode_blocks(a.E);
    hipLaunchKernelGGL(k_episode, dim3((unsigned)nb), dim3(kEpisodeBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_episode_finish, dim3(1), dim3(kEpisodeBlock), 0, s, a, (int)nb);
    return hipGetLastError();
}

}  // namespace f110
