// f110_learner_args.h — the learner's data side: the n-step row rule, the prioritized replay ring,
// the n-step window in front of it and flat Adam, with their launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"
#include "f110_repeat.h"

namespace f110 {

// ------------------------------------------------------- n-step returns --
// One env's push into its n-step window (the semantics of include/f110.h, "n-step returns";
// k_nstep_update and f110_host_nstep both call it).  The window is a ring of n slots: its len
// pending entries sit at slots (head + i) % n, oldest first, each with a running return ret (f64)
// and a reward count k; pw[i] = gamma^i as sequential products (pw[0] = 1).  r is this step's
// reward.  Returns the number of emitted rows (0..n), oldest first; for row j
//   e_slot[j]   the window slot that holds its (obs, act), or -1: this push's own (s, a);
//   e_reward[j] (float)ret;  e_done[j] the effective done, 1 - gamma^(k-1) (1 - done).
// store = the slot this push's (s, a) is to be written to, or -1 when it does not stay pending
// (a reset row, or emitted by this very push).  A slot that is emitted is never the slot stored
// to in the same push: the caller may move the rows of one push in any order.
F110_HD int nstep_update(int n, const double *pw, double r, int term, int trunc, int was_reset, int32_t &len,
                         int32_t &head, double *ret, int32_t *k, int32_t *e_slot, float *e_reward, float *e_done,
                         int32_t &store) {
    store = -1;
    if (was_reset) {  // not a transition: whatever is pending belongs to an episode that is over
        len = 0;
        head = 0;
        return 0;
    }
    int s = head;
    for (int i = 0; i < len; ++i) {
        const double p = pw[k[s]] * r;  // (product and sum kept apart: no FMA)
        ret[s] = ret[s] + p;
        k[s] += 1;
        s = s + 1 == n ? 0 : s + 1;
    }
    const int ns = s;  // (head + len) % n: len < n before a push
    ret[ns] = r;       // assigned, not 0.0 + r: -0.0 survives
    k[ns] = 1;
    len += 1;
    if (term || trunc) {  // the episode ends: every pending entry leaves, with what it has
        const int cnt = len;
        s = head;
        for (int j = 0; j < cnt; ++j) {
            e_slot[j] = s == ns ? -1 : s;
            e_reward[j] = (float)ret[s];
            e_done[j] = term ? 1.0f : (float)(1.0 - pw[k[s] - 1]);
            s = s + 1 == n ? 0 : s + 1;
        }
        len = 0;
        head = 0;
        return cnt;
    }
    if (len == n) {  // the oldest entry has its n rewards
        e_slot[0] = head == ns ? -1 : head;
        e_reward[0] = (float)ret[head];
        e_done[0] = (float)(1.0 - pw[n - 1]);
        if (head != ns) store = ns;  // (n == 1: the new entry itself left)
        head = head + 1 == n ? 0 : head + 1;
        len -= 1;
        return 1;
    }
    store = ns;
    return 0;
}

// ---- prioritized replay (f110_replay.hip) ---------------------------------
constexpr int kTieCap = 4096;        // keys equal to the selection threshold kept for the tie break
constexpr int kReplayMaxGrid = 1024; // blocks of the streaming replay kernels
constexpr int kReplayMaxBatch = 8192;
// Copies of the radix select's global histograms: block b adds into copy b % kHistRep (consecutive
// blocks land on different XCDs), so each bin's device-scope atomics are spread over 8 addresses;
// the consumer sums the copies.  Layout hist[(copy * 4 + pass) * 256 + bin].
constexpr int kHistRep = 8;

// Device header of a replay buffer (one per f110_replay).
struct ReplayHdr {
    int64_t length;     // PrioritizedExperienceReplayBuffer._length
    int64_t next;       // _next_idx
    uint64_t draws;     // sample() calls so far (Philox counter)
    double den;         // sum of (p + eps)^alpha at the last sample
    int32_t replace;    // the last sample drew with replacement
    int32_t pad0_;
    uint32_t prefix;    // radix select: threshold key so far
    uint32_t kleft;     //   rank still to select below/at the prefix
    uint32_t n_lt, n_tie;  // keys below / equal to the threshold (n_tie zeroed by k_finish)
    uint32_t overflow;  // samples whose tie list overflowed kTieCap (k_finish then walks the keys itself)
    uint32_t pad_;
    uint32_t sel_prefix[4], sel_kleft[4];  // the select through digit q (written by the kernel after
                                           // pass q's histogram, read by the next one)
};

struct ReplayView {
    ReplayHdr *hdr;
    int64_t capacity;
    int32_t obs_dim, act_dim;
    float *obs, *next_obs, *act, *reward, *done, *prio;  // [cap][D], [cap][D], [cap][A], [cap] x3
    double *wt;          // [cap] sampling weight (prio + eps)^alpha, written with prio (add, update)
    uint32_t *keys;      // [cap] exponential-race keys
    uint32_t *hist;      // [4][256]
    double *den_part;    // [kReplayMaxGrid]
    uint32_t *part;      // [kReplayMaxGrid] per-block max priority (add) / selected count (sample)
    uint64_t *sel;       // [kReplayMaxBatch] indices of the keys below the threshold, in index order
    uint32_t *tie;       // [kTieCap]
    int64_t *pos;        // [max rows per add] ring slot of each added row (-1: not stored)
    double alpha;
    float eps;           // the buffer's priority_epsilon (replay_buffer.py:24, 88)
    uint64_t seed;
};

struct ReplayRows {      // one add(): n transitions (device, f32 rows with strides in floats)
    const float *obs, *next_obs, *act, *reward;
    const double *reward64; // [n] f64 rewards instead of reward (rounded to f32 as .to(torch.float32))
    const float *priority;  // [n] explicit priorities or null (= the max priority)
    const uint8_t *done;
    int64_t obs_stride, next_stride, act_stride;
    int32_t vec4;        // rows 16-B aligned and obs_dim % 4 == 0
};

struct ReplayBatch {     // one sample(): the gathered batch (device, contiguous)
    float *obs, *next_obs, *act, *reward, *done;
    int32_t vec4;
};

hipError_t launch_replay_add_index(const ReplayView &v, const uint8_t *mask, int mask_skip, const float *priority,
                                   int64_t n, hipStream_t s);  // ring slots, priorities, header
hipError_t launch_replay_add_copy(const ReplayView &v, const ReplayRows &in, int64_t n, hipStream_t s);  // the rows
hipError_t launch_replay_select(const ReplayView &v, int32_t batch, double beta, int64_t *idx, float *w,
                                bool known_full, hipStream_t s);  // idx / weights (reads no row data)
hipError_t launch_replay_select_keys(const ReplayView &v, int32_t batch, double beta, int64_t *idx, float *w,
                                     hipStream_t s);  // the same select over given v.keys (length >= batch)
hipError_t launch_replay_gather(const ReplayView &v, int32_t batch, const int64_t *idx, const ReplayBatch &out,
                                hipStream_t s);
hipError_t launch_replay_update(const ReplayView &v, const int64_t *idx, const float *val, int64_t n, float add_eps,
                                int32_t from_td, int32_t serial, hipStream_t s);
hipError_t prepare_replay(int32_t max_batch);
int replay_grid(int64_t capacity);

// ---- n-step accumulator in front of the ring (f110_replay.hip) -------------
constexpr int kNstepMax = 16;
struct NstepView {       // one f110_nstep (device)
    int64_t n_envs;
    int32_t n, obs_dim, act_dim;
    const double *pw;    // [n + 1] gamma^i, sequential products
    int32_t *len, *head; // [N] pending entries, slot of the oldest
    double *ret;         // [N][n] running returns
    int32_t *k;          // [N][n] rewards in ret
    float *obs, *act;    // [N][n][D], [N][n][A] the pending entries' rows
    // one push's scratch
    int32_t *cnt;        // [N] rows the env emits
    int32_t *store;      // [N] window slot this push's (s, a) goes to, or -1
    int64_t *base;       // [N] ring slot of the env's first emitted row
    int32_t *e_slot;     // [N][n] window slot of emitted row j (-1: this push's own row)
    float *e_reward, *e_done;  // [N][n]
};

struct NstepRows {       // one push: n_envs raw step outputs (device)
    const float *obs, *act, *next_obs;
    const double *reward;
    const uint8_t *terminated, *truncated, *was_reset;  // truncated may be null
    int64_t obs_stride, act_stride, next_stride;
    int32_t vec4;        // every row moved is 16-B aligned and obs_dim % 4 == 0
};

hipError_t launch_nstep_push(const ReplayView &v, const NstepView &w, const NstepRows &in, hipStream_t s);
hipError_t launch_nstep_reset(const NstepView &w, const uint8_t *env_mask, hipStream_t s);

// ---- action repeat around the env step (f110_replay.hip) -------------------
// What the ring-slot scan reads and writes (k_count_scan, f110_replay.hip): a row count per env in,
// the ring slot of each env's first row out.  NstepView and RepeatView both supply one.
struct CountView {
    int64_t n_envs;
    const int32_t *cnt;  // [N] rows the env emits
    int64_t *base;       // [N] ring slot of the env's first emitted row
};

struct RepeatView {      // one f110_repeat (device)
    int64_t n_envs;
    int32_t repeat, obs_dim, act_dim;
    const double *pw;    // [repeat + 1] gamma^i, sequential products
    int32_t *k;          // [N] phase
    double *ret;         // [N] running return
    float *obs, *act;    // [N][D], [N][A] the block's first observation and its action
    // one push's scratch
    int32_t *cnt;        // [N] 1: the env's block leaves
    int64_t *base;       // [N] its ring slot
    float *e_reward, *e_done;  // [N]
};

struct RepeatHold {      // one hold: the policy's inputs and outputs of n_envs envs (device)
    const float *obs;
    float *act;          // in / out
    uint8_t *decision;   // [N] or null
    int64_t obs_stride, act_stride;
    int32_t vec4;        // obs rows 16-B aligned and obs_dim % 4 == 0
};

struct RepeatRows {      // one push: n_envs raw step outputs (device)
    const float *next_obs;
    const double *reward;
    const uint8_t *terminated, *truncated, *was_reset;  // truncated may be null
    int64_t next_stride;
    int32_t vec4;        // next_obs rows 16-B aligned and obs_dim % 4 == 0
};

hipError_t launch_repeat_hold(const RepeatView &w, const RepeatHold &in, hipStream_t s);
hipError_t launch_repeat_push(const ReplayView &v, const RepeatView &w, const RepeatRows &in, hipStream_t s);
hipError_t launch_repeat_reset(const RepeatView &w, const uint8_t *env_mask, hipStream_t s);

// ---- flat Adam (f110_adam.hip) --------------------------------------------
struct AdamArgs {
    float *param, *exp_avg, *exp_avg_sq;
    const float *grad;
    int64_t n;
    double lr, beta1, beta2, eps;
    int64_t *step;     // device step counter
    uint32_t *done;    // device: blocks finished (last one advances step)
    float *target;     // the target network's flat buffer (soft update after the step) or null
    float tau;
};
hipError_t launch_adam(const AdamArgs &a, hipStream_t s);

}  // namespace f110
