// f110_replay_capi.cpp — host side of the learner's device components
// (include/f110.h, "prioritized experience replay", "n-step returns", "action
// repeat" and "learner optimizer"): argument checks, the device allocation at
// create, the launches of f110_replay.hip / f110_adam.hip.  (The n-step and
// action-repeat host models, f110_host_nstep and f110_host_repeat_*, and the
// argument checks they share are in f110_host.cpp.)
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/f110.h"
#include "f110_host.h"
#include "f110_host_util.h"
#include "f110_learner_args.h"

using namespace f110;

struct f110_replay {
    DeviceArena arena;
    int64_t max_add = 0;
    int32_t max_batch = 0;
    int64_t known_len = 0;  // a lower bound of the device length seen by f110_replay_length (never shrinks)
    ReplayView v{};

    // n elements and 16 bytes of slack (the vectorised row copies), not cleared
    template <class T>
    hipError_t alloc(T **p, size_t n) {
        return arena.alloc(p, n, /*zero=*/false, 16);
    }
};

extern "C" int f110_replay_create(f110_replay **out, int32_t device, int64_t capacity, int32_t obs_dim,
                                  int32_t act_dim, int32_t max_batch, int64_t max_add, double alpha, double eps,
                                  uint64_t seed) {
    if (!out || capacity <= 0 || capacity >= (int64_t)1 << 32 || obs_dim <= 0 || act_dim <= 0 || act_dim > 256 ||
        max_batch <= 0 || max_batch > kReplayMaxBatch || max_add <= 0 || max_add > capacity)
        return fail(F110_E_INVALID,
                    "f110_replay_create: bad arguments (0 < capacity < 2^32, 0 < act_dim <= 256, "
                    "0 < max_batch <= 8192, 0 < max_add <= capacity)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(F110_E_NODEVICE, "f110_replay_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(F110_E_NODEVICE, "f110_replay_create: hipSetDevice");
    auto *rb = new f110_replay();
    rb->arena.device = device;
    rb->max_add = max_add;
    rb->max_batch = max_batch;
    ReplayView &v = rb->v;
    v.capacity = capacity;
    v.obs_dim = obs_dim;
    v.act_dim = act_dim;
    v.alpha = alpha;
    v.eps = (float)eps;  // ps + self._eps is evaluated in float32 (NEP 50)
    v.seed = seed;
    const size_t cap = (size_t)capacity;
    hipError_t e = rb->alloc(&v.hdr, 1);
    if (e == hipSuccess) e = rb->alloc(&v.obs, cap * obs_dim);
    if (e == hipSuccess) e = rb->alloc(&v.next_obs, cap * obs_dim);
    if (e == hipSuccess) e = rb->alloc(&v.act, cap * act_dim);
    if (e == hipSuccess) e = rb->alloc(&v.reward, cap);
    if (e == hipSuccess) e = rb->alloc(&v.done, cap);
    if (e == hipSuccess) e = rb->alloc(&v.prio, cap);
    if (e == hipSuccess) e = rb->alloc(&v.wt, cap);
    if (e == hipSuccess) e = rb->alloc(&v.keys, cap);
    if (e == hipSuccess) e = rb->alloc(&v.hist, (size_t)kHistRep * 4 * 256);
    if (e == hipSuccess) e = rb->alloc(&v.den_part, kReplayMaxGrid);
    if (e == hipSuccess) e = rb->alloc(&v.part, kReplayMaxGrid);
    if (e == hipSuccess) e = rb->alloc(&v.sel, kReplayMaxBatch);
    if (e == hipSuccess) e = rb->alloc(&v.tie, kTieCap);
    if (e == hipSuccess) e = rb->alloc(&v.pos, (size_t)max_add);
    if (e == hipSuccess) e = hipMemset(v.hdr, 0, sizeof(ReplayHdr));
    if (e == hipSuccess) e = hipMemset(v.prio, 0, cap * sizeof(float));
    if (e == hipSuccess) e = hipMemset(v.wt, 0, cap * sizeof(double));
    if (e == hipSuccess) e = hipMemset(v.hist, 0, (size_t)kHistRep * 4 * 256 * sizeof(uint32_t));
    if (e == hipSuccess) e = prepare_replay(max_batch);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete rb;  // (the arena frees what was allocated)
        return hip_fail("f110_replay_create", e, F110_E_ALLOC);
    }
    *out = rb;
    return F110_OK;
}

extern "C" int f110_replay_destroy(f110_replay *rb) {
    delete rb;
    return F110_OK;
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

namespace {
int replay_add(f110_replay *rb, const char *fn, const float *obs, int64_t obs_stride, const float *act,
               int64_t act_stride, const float *reward, const double *reward64, const float *next_obs,
               int64_t next_stride, const uint8_t *done, const float *priority, const uint8_t *mask, int mask_skip,
               int64_t n, void *stream) {
    if (!rb) return fail(F110_E_INVALID, std::string(fn) + ": null buffer");
    if (n < 0 || n > rb->max_add) return fail(F110_E_INVALID, std::string(fn) + ": n must be in [0, max_add]");
    if (n == 0) return F110_OK;
    const ReplayView &v = rb->v;
    if (!obs || !act || (!reward && !reward64) || !next_obs || obs_stride < v.obs_dim || next_stride < v.obs_dim ||
        act_stride < v.act_dim)
        return fail(F110_E_INVALID, std::string(fn) + ": null row pointer or stride below the row length");
    if (hipSetDevice(rb->arena.device) != hipSuccess) return fail(F110_E_HIP, std::string(fn) + ": hipSetDevice");
    ReplayRows in{};
    in.obs = obs;
    in.next_obs = next_obs;
    in.act = act;
    in.reward = reward;
    in.reward64 = reward64;
    in.done = done;
    in.priority = priority;
    in.obs_stride = obs_stride;
    in.next_stride = next_stride;
    in.act_stride = act_stride;
    in.vec4 = (v.obs_dim % 4 == 0 && obs_stride % 4 == 0 && next_stride % 4 == 0 && aligned16(obs) &&
               aligned16(next_obs)) ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_replay_add_index(v, mask, mask_skip, priority, n, s);
    if (e == hipSuccess) e = launch_replay_add_copy(v, in, n, s);
    if (e != hipSuccess) return hip_fail(fn, e);
    return F110_OK;
}
}  // namespace

extern "C" int f110_replay_add(f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                               int64_t act_stride, const float *reward, const float *next_obs, int64_t next_stride,
                               const uint8_t *done, const float *priority, const uint8_t *mask, int64_t n,
                               void *stream) {
    return replay_add(rb, "f110_replay_add", obs, obs_stride, act, act_stride, reward, nullptr, next_obs, next_stride,
                      done, priority, mask, 0, n, stream);
}

extern "C" int f110_replay_add_env(f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                                   int64_t act_stride, const double *reward, const float *next_obs,
                                   int64_t next_stride, const uint8_t *terminated, const uint8_t *was_reset,
                                   int64_t n, void *stream) {
    if (!reward) return fail(F110_E_INVALID, "f110_replay_add_env: null reward");
    return replay_add(rb, "f110_replay_add_env", obs, obs_stride, act, act_stride, nullptr, reward, next_obs,
                      next_stride, terminated, nullptr, was_reset, 1, n, stream);
}

extern "C" int f110_replay_sample(f110_replay *rb, int32_t batch, double beta, int64_t *idx, float *weights,
                                  float *obs, float *act, float *reward, float *next_obs, float *done,
                                  void *stream) {
    if (!rb || !idx || !weights) return fail(F110_E_INVALID, "f110_replay_sample: null argument");
    if (batch <= 0 || batch > rb->max_batch) return fail(F110_E_INVALID, "f110_replay_sample: batch must be in [1, max_batch]");
    if (obs && (!act || !reward || !next_obs || !done))
        return fail(F110_E_INVALID, "f110_replay_sample: give all batch outputs or none");
    if (hipSetDevice(rb->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_replay_sample: hipSetDevice");
    ReplayBatch out{};
    out.obs = obs;
    out.next_obs = next_obs;
    out.act = act;
    out.reward = reward;
    out.done = done;
    out.vec4 = (rb->v.obs_dim % 4 == 0 && obs && aligned16(obs) && aligned16(next_obs)) ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_replay_select(rb->v, batch, beta, idx, weights, rb->known_len >= batch, s);
    if (e == hipSuccess) e = launch_replay_gather(rb->v, batch, idx, out, s);
    if (e != hipSuccess) return hip_fail("f110_replay_sample", e);
    return F110_OK;
}

// Test hook: the select of f110_replay_sample over keys the caller chooses (no draw, no gather).
extern "C" int f110_replay_select_keys(f110_replay *rb, const uint32_t *keys, int64_t n, int32_t batch, double beta,
                                       int64_t *idx, float *weights, void *stream) {
    if (!rb || !keys || !idx || !weights) return fail(F110_E_INVALID, "f110_replay_select_keys: null argument");
    if (batch <= 0 || batch > rb->max_batch)
        return fail(F110_E_INVALID, "f110_replay_select_keys: batch must be in [1, max_batch]");
    int64_t len = 0;
    const int rc = f110_replay_length(rb, &len, nullptr, stream);
    if (rc != F110_OK) return rc;
    if (n != len || batch > n)
        return fail(F110_E_INVALID, "f110_replay_select_keys: n must be the buffer's length and batch <= n");
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(rb->v.keys, keys, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = launch_replay_select_keys(rb->v, batch, beta, idx, weights, s);
    if (e != hipSuccess) return hip_fail("f110_replay_select_keys", e);
    return F110_OK;
}

extern "C" int f110_replay_update_priorities(f110_replay *rb, const int64_t *idx, const float *values, int64_t n,
                                             int32_t from_td, float add_eps, void *stream) {
    if (!rb || n < 0 || (n > 0 && (!idx || !values)))
        return fail(F110_E_INVALID, "f110_replay_update_priorities: bad arguments");
    if (hipSetDevice(rb->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_replay_update_priorities: hipSetDevice");
    hipError_t e = launch_replay_update(rb->v, idx, values, n, add_eps, from_td ? 1 : 0, 0, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_replay_update_priorities", e);
    return F110_OK;
}

extern "C" int f110_replay_length(f110_replay *rb, int64_t *length, int64_t *next_idx, void *stream) {
    if (!rb) return fail(F110_E_INVALID, "f110_replay_length: null buffer");
    if (hipSetDevice(rb->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_replay_length: hipSetDevice");
    ReplayHdr h{};
    hipError_t e = hipMemcpyAsync(&h, rb->v.hdr, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_replay_length", e);
    if (length) *length = h.length;
    if (next_idx) *next_idx = h.next;
    if (h.length > rb->known_len) rb->known_len = h.length;  // the ring never shrinks
    return F110_OK;
}

extern "C" int f110_replay_arrays(f110_replay *rb, float **priority, float **obs, float **act, float **reward,
                                  float **next_obs, float **done) {
    if (!rb) return fail(F110_E_INVALID, "f110_replay_arrays: null buffer");
    if (priority) *priority = rb->v.prio;
    if (obs) *obs = rb->v.obs;
    if (act) *act = rb->v.act;
    if (reward) *reward = rb->v.reward;
    if (next_obs) *next_obs = rb->v.next_obs;
    if (done) *done = rb->v.done;
    return F110_OK;
}

extern "C" int f110_replay_select_state(f110_replay *rb, uint32_t **keys, double **wt, uint32_t *prefix,
                                        uint32_t *kleft, uint32_t *n_lt, double *den, uint32_t *overflow,
                                        void *stream) {
    if (!rb) return fail(F110_E_INVALID, "f110_replay_select_state: null buffer");
    if (keys) *keys = rb->v.keys;
    if (wt) *wt = rb->v.wt;
    if (!prefix && !kleft && !n_lt && !den && !overflow) return F110_OK;
    if (hipSetDevice(rb->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_replay_select_state: hipSetDevice");
    ReplayHdr h{};
    hipError_t e = hipMemcpyAsync(&h, rb->v.hdr, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_replay_select_state", e);
    if (prefix) *prefix = h.prefix;
    if (kleft) *kleft = h.kleft;
    if (n_lt) *n_lt = h.n_lt;
    if (den) *den = h.den;
    if (overflow) *overflow = h.overflow;
    return F110_OK;
}

// ---- n-step accumulator -------------------------------------------------------
struct f110_nstep {
    DeviceArena arena;
    NstepView w{};

    // n elements and 16 bytes of slack (the vectorised row copies), all zero
    template <class T>
    hipError_t alloc(T **p, size_t n) {
        return arena.alloc(p, n, /*zero=*/true, 16);
    }
};

extern "C" int f110_nstep_create(f110_nstep **out, int32_t device, int64_t n_envs, int32_t n_step, double gamma,
                                 int32_t obs_dim, int32_t act_dim) {
    if (!out) return fail(F110_E_INVALID, "f110_nstep_create: null out");
    const int rc = check_nstep_args("f110_nstep_create", n_envs, n_step, gamma, obs_dim, act_dim);
    if (rc != F110_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(F110_E_NODEVICE, "f110_nstep_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(F110_E_NODEVICE, "f110_nstep_create: hipSetDevice");
    auto *ns = new f110_nstep();
    ns->arena.device = device;
    NstepView &w = ns->w;
    w.n_envs = n_envs;
    w.n = n_step;
    w.obs_dim = obs_dim;
    w.act_dim = act_dim;
    const size_t N = (size_t)n_envs, W = N * (size_t)n_step;
    double pw[kNstepMax + 1];
    nstep_powers(gamma, n_step, pw);
    double *dpw = nullptr;
    hipError_t e = ns->alloc(&dpw, (size_t)n_step + 1);
    w.pw = dpw;
    if (e == hipSuccess) e = ns->alloc(&w.len, N);
    if (e == hipSuccess) e = ns->alloc(&w.head, N);
    if (e == hipSuccess) e = ns->alloc(&w.ret, W);
    if (e == hipSuccess) e = ns->alloc(&w.k, W);
    if (e == hipSuccess) e = ns->alloc(&w.obs, W * obs_dim);
    if (e == hipSuccess) e = ns->alloc(&w.act, W * act_dim);
    if (e == hipSuccess) e = ns->alloc(&w.cnt, N);
    if (e == hipSuccess) e = ns->alloc(&w.store, N);
    if (e == hipSuccess) e = ns->alloc(&w.base, N);
    if (e == hipSuccess) e = ns->alloc(&w.e_slot, W);
    if (e == hipSuccess) e = ns->alloc(&w.e_reward, W);
    if (e == hipSuccess) e = ns->alloc(&w.e_done, W);
    if (e == hipSuccess) e = hipMemcpy(dpw, pw, ((size_t)n_step + 1) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete ns;  // (the arena frees what was allocated)
        return hip_fail("f110_nstep_create", e, F110_E_ALLOC);
    }
    *out = ns;
    return F110_OK;
}

extern "C" int f110_nstep_destroy(f110_nstep *ns) {
    delete ns;
    return F110_OK;
}

extern "C" int f110_nstep_push(f110_nstep *ns, f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                               int64_t act_stride, const double *reward, const float *next_obs, int64_t next_stride,
                               const uint8_t *terminated, const uint8_t *truncated, const uint8_t *was_reset,
                               void *stream) {
    if (!ns || !rb) return fail(F110_E_INVALID, "f110_nstep_push: null accumulator or buffer");
    const NstepView &w = ns->w;
    const ReplayView &v = rb->v;
    if (ns->arena.device != rb->arena.device) return fail(F110_E_INVALID, "f110_nstep_push: accumulator and buffer on different devices");
    if (w.obs_dim != v.obs_dim || w.act_dim != v.act_dim)
        return fail(F110_E_INVALID, "f110_nstep_push: obs_dim / act_dim differ from the replay's");
    const int rc = check_nstep_capacity("f110_nstep_push", w.n_envs, w.n, v.capacity);
    if (rc != F110_OK) return rc;
    if (!obs || !act || !reward || !next_obs || !terminated || !was_reset || obs_stride < v.obs_dim ||
        next_stride < v.obs_dim || act_stride < v.act_dim)
        return fail(F110_E_INVALID, "f110_nstep_push: null row pointer or stride below the row length");
    if (hipSetDevice(ns->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_nstep_push: hipSetDevice");
    NstepRows in{};
    in.obs = obs;
    in.act = act;
    in.next_obs = next_obs;
    in.reward = reward;
    in.terminated = terminated;
    in.truncated = truncated;
    in.was_reset = was_reset;
    in.obs_stride = obs_stride;
    in.act_stride = act_stride;
    in.next_stride = next_stride;
    // (the window's and the ring's rows start 16-B aligned whenever obs_dim % 4 == 0)
    in.vec4 = (v.obs_dim % 4 == 0 && obs_stride % 4 == 0 && next_stride % 4 == 0 && aligned16(obs) &&
               aligned16(next_obs)) ? 1 : 0;
    hipError_t e = launch_nstep_push(v, w, in, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_nstep_push", e);
    return F110_OK;
}

extern "C" int f110_nstep_reset(f110_nstep *ns, const uint8_t *env_mask, void *stream) {
    if (!ns) return fail(F110_E_INVALID, "f110_nstep_reset: null accumulator");
    if (hipSetDevice(ns->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_nstep_reset: hipSetDevice");
    hipError_t e = launch_nstep_reset(ns->w, env_mask, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_nstep_reset", e);
    return F110_OK;
}

extern "C" int f110_nstep_arrays(f110_nstep *ns, int32_t **len, int32_t **head, double **ret, int32_t **k, float **obs,
                                 float **act) {
    if (!ns) return fail(F110_E_INVALID, "f110_nstep_arrays: null accumulator");
    if (len) *len = ns->w.len;
    if (head) *head = ns->w.head;
    if (ret) *ret = ns->w.ret;
    if (k) *k = ns->w.k;
    if (obs) *obs = ns->w.obs;
    if (act) *act = ns->w.act;
    return F110_OK;
}

// ---- action repeat --------------------------------------------------------------
struct f110_repeat {
    DeviceArena arena;
    RepeatView w{};

    // n elements and 16 bytes of slack (the vectorised row copies), all zero
    template <class T>
    hipError_t alloc(T **p, size_t n) {
        return arena.alloc(p, n, /*zero=*/true, 16);
    }
};

extern "C" int f110_repeat_create(f110_repeat **out, int32_t device, int64_t n_envs, int32_t repeat, double gamma,
                                  int32_t obs_dim, int32_t act_dim) {
    if (!out) return fail(F110_E_INVALID, "f110_repeat_create: null out");
    const int rc = check_repeat_args("f110_repeat_create", n_envs, repeat, gamma, obs_dim, act_dim);
    if (rc != F110_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(F110_E_NODEVICE, "f110_repeat_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(F110_E_NODEVICE, "f110_repeat_create: hipSetDevice");
    auto *rp = new f110_repeat();
    rp->arena.device = device;
    RepeatView &w = rp->w;
    w.n_envs = n_envs;
    w.repeat = repeat;
    w.obs_dim = obs_dim;
    w.act_dim = act_dim;
    const size_t N = (size_t)n_envs;
    double pw[kRepeatMax + 1];
    nstep_powers(gamma, repeat, pw);
    double *dpw = nullptr;
    hipError_t e = rp->alloc(&dpw, (size_t)repeat + 1);
    w.pw = dpw;
    if (e == hipSuccess) e = rp->alloc(&w.k, N);
    if (e == hipSuccess) e = rp->alloc(&w.ret, N);
    if (e == hipSuccess) e = rp->alloc(&w.obs, N * obs_dim);
    if (e == hipSuccess) e = rp->alloc(&w.act, N * act_dim);
    if (e == hipSuccess) e = rp->alloc(&w.cnt, N);
    if (e == hipSuccess) e = rp->alloc(&w.base, N);
    if (e == hipSuccess) e = rp->alloc(&w.e_reward, N);
    if (e == hipSuccess) e = rp->alloc(&w.e_done, N);
    if (e == hipSuccess) e = hipMemcpy(dpw, pw, ((size_t)repeat + 1) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete rp;  // (the arena frees what was allocated)
        return hip_fail("f110_repeat_create", e, F110_E_ALLOC);
    }
    *out = rp;
    return F110_OK;
}

extern "C" int f110_repeat_destroy(f110_repeat *rp) {
    delete rp;
    return F110_OK;
}

extern "C" int f110_repeat_hold(f110_repeat *rp, const float *obs, int64_t obs_stride, float *act, int64_t act_stride,
                                uint8_t *decision, void *stream) {
    if (!rp) return fail(F110_E_INVALID, "f110_repeat_hold: null handle");
    const RepeatView &w = rp->w;
    if (!obs || !act || obs_stride < w.obs_dim || act_stride < w.act_dim)
        return fail(F110_E_INVALID, "f110_repeat_hold: null row pointer or stride below the row length");
    if (hipSetDevice(rp->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_repeat_hold: hipSetDevice");
    RepeatHold in{};
    in.obs = obs;
    in.act = act;
    in.decision = decision;
    in.obs_stride = obs_stride;
    in.act_stride = act_stride;
    // (the latched rows start 16-B aligned whenever obs_dim % 4 == 0)
    in.vec4 = (w.obs_dim % 4 == 0 && obs_stride % 4 == 0 && aligned16(obs)) ? 1 : 0;
    hipError_t e = launch_repeat_hold(w, in, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_repeat_hold", e);
    return F110_OK;
}

extern "C" int f110_repeat_push(f110_repeat *rp, f110_replay *rb, const double *reward, const float *next_obs,
                                int64_t next_stride, const uint8_t *terminated, const uint8_t *truncated,
                                const uint8_t *was_reset, void *stream) {
    if (!rp || !rb) return fail(F110_E_INVALID, "f110_repeat_push: null handle or buffer");
    const RepeatView &w = rp->w;
    const ReplayView &v = rb->v;
    if (rp->arena.device != rb->arena.device) return fail(F110_E_INVALID, "f110_repeat_push: handle and buffer on different devices");
    if (w.obs_dim != v.obs_dim || w.act_dim != v.act_dim)
        return fail(F110_E_INVALID, "f110_repeat_push: obs_dim / act_dim differ from the replay's");
    const int rc = check_repeat_capacity("f110_repeat_push", w.n_envs, v.capacity);
    if (rc != F110_OK) return rc;
    if (!reward || !next_obs || !terminated || !was_reset || next_stride < v.obs_dim)
        return fail(F110_E_INVALID, "f110_repeat_push: null pointer or stride below the row length");
    if (hipSetDevice(rp->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_repeat_push: hipSetDevice");
    RepeatRows in{};
    in.next_obs = next_obs;
    in.reward = reward;
    in.terminated = terminated;
    in.truncated = truncated;
    in.was_reset = was_reset;
    in.next_stride = next_stride;
    // (the latched and the ring's rows start 16-B aligned whenever obs_dim % 4 == 0)
    in.vec4 = (v.obs_dim % 4 == 0 && next_stride % 4 == 0 && aligned16(next_obs)) ? 1 : 0;
    hipError_t e = launch_repeat_push(v, w, in, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_repeat_push", e);
    return F110_OK;
}

extern "C" int f110_repeat_reset(f110_repeat *rp, const uint8_t *env_mask, void *stream) {
    if (!rp) return fail(F110_E_INVALID, "f110_repeat_reset: null handle");
    if (hipSetDevice(rp->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_repeat_reset: hipSetDevice");
    hipError_t e = launch_repeat_reset(rp->w, env_mask, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_repeat_reset", e);
    return F110_OK;
}

extern "C" int f110_repeat_arrays(f110_repeat *rp, int32_t **k, double **ret, float **obs, float **act) {
    if (!rp) return fail(F110_E_INVALID, "f110_repeat_arrays: null handle");
    if (k) *k = rp->w.k;
    if (ret) *ret = rp->w.ret;
    if (obs) *obs = rp->w.obs;
    if (act) *act = rp->w.act;
    return F110_OK;
}

extern "C" int f110_adam_step(float *param, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t n,
                              double lr, double beta1, double beta2, double eps, void *state, float *target,
                              double tau, void *stream) {
    if (n < 0 || (n > 0 && (!param || !exp_avg || !exp_avg_sq || !grad || !state)))
        return fail(F110_E_INVALID, "f110_adam_step: bad arguments");
    AdamArgs a{};
    a.param = param;
    a.exp_avg = exp_avg;
    a.exp_avg_sq = exp_avg_sq;
    a.grad = grad;
    a.n = n;
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.step = static_cast<int64_t *>(state);
    a.target = target;
    a.tau = (float)tau;
    a.done = reinterpret_cast<uint32_t *>(static_cast<int64_t *>(state) + 1);
    hipError_t e = launch_adam(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_adam_step", e);
    return F110_OK;
}
