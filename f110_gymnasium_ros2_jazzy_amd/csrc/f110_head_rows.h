// f110_head_rows.h — what the learner-head translation units share (private; f110_ddpg.hip,
// f110_td3.hip and f110_selfplay.hip): the launch geometry of the row-per-half-wave kernels, the row dot product and
// its backward, the deterministic sums, the exploration draw and the argument checks, and ahead of
// them the row rules that the kernels share with the host hooks of these files (explore_one,
// td3_smooth_one, td3_row).  All but the row rules sits in an anonymous namespace: each translation
// unit gets its own copy, inlined into its kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/f110.h"
#include "f110_host_util.h"
#include "f110_math.h"
#include "f110_rng.h"

namespace f110 {

// ---------------------------------------------------- exploration head rows --
// One output of one row of f110_ddpg_actor_explore_env (include/f110.h; k_head_fwd's kExploreEnv
// epilogue and f110_host_explore_rows both call it): act the deterministic action, n the N(0,1) draw,
// x the OU state of (row, output) (kind 1; unused for kind 0).  sqdt = sqrt(dt), taken on the host
// once (np.sqrt(self.dt)).  Returns the action.
//   reset  zeroes x first, on every row;
//   eval   the action is act, no draw used, x untouched (agent.py `if not training: return action`);
//   kind 0 GaussianActionNoise.__call__ (agent.py:520-539) in f32, kExplore's operations;
//   kind 1 OUActionNoise.__call__ (agent.py:490-505) in f64, left to right, no FMA: the state is
//          float64 after its first call, the draw a float32 (mu = 0: the first call's float32 drift
//          is an exact 0 either way).
constexpr int kExploreGaussian = 0, kExploreOU = 1;

F110_HD float explore_one(int kind, float act, float n, double sigma, double theta, double mu, double dt, double sqdt,
                          bool reset, bool eval, float lo, float hi, double &x) {
    if (reset) x = 0.0;
    if (eval) return act;
    if (kind == kExploreGaussian) {
        float v = act + (float)sigma * n;
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
        return v;
    }
    const double dx = theta * (mu - x) * dt + (sigma * sqdt) * (double)n;
    x = x + dx;
    return (float)clip((double)act + x, (double)lo, (double)hi);
}

// ---------------------------------------------------------------- TD3 rows --
// The two row rules of the TD3 learner (include/f110.h, "TD3 heads"; k_td3_target_action /
// k_td3_critic_step and f110_host_td3_smooth_rows / f110_host_td3_rows call them).  f32, left to
// right, no FMA.
//
// Target-policy smoothing of one output: act the target actor's action, n the N(0,1) draw,
// scale_j the actor's half-range 0.5 * (high - low) of this output, so policy_noise and noise_clip
// are in units of the tanh output (the action box is asymmetric: steer +-0.4189, speed 0..20).
// NaN stays NaN.
F110_HD float td3_smooth_one(float act, float n, float policy_noise, float noise_clip, float scale_j, float lo,
                             float hi) {
    const float s = policy_noise * scale_j;
    const float c = noise_clip * scale_j;
    float e = s * n;
    e = e < -c ? -c : e;
    e = e > c ? c : e;
    float v = act + e;
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return v;
}

// One row of the twin critic update: clipped double-Q target (torch.minimum of the two target
// critics, NaN propagates), the two TD errors and their loss gradients (k_critic_step's operations,
// gb = g / B), the PER priority and the row's loss term.
F110_HD void td3_row(float r, float d, float gamma, float q1t, float q2t, float q1, float q2, float w, float gb,
                     float &td1, float &td2, float &dq1, float &dq2, float &prio, float &wl) {
    const float m = (q2t < q1t || q2t != q2t) ? q2t : q1t;
    const float y = r + (gamma * (1.0f - d)) * m;
    td1 = y - q1;
    td2 = y - q2;
    dq1 = -((gb * w) * (2.0f * td1));
    dq2 = -((gb * w) * (2.0f * td2));
    prio = 0.5f * (fabsf(td1) + fabsf(td2));
    wl = w * (td1 * td1) + w * (td2 * td2);
}

namespace {

constexpr int kHB = 256;      // threads per block
constexpr int kRowLanes = 32; // lanes per row (a half-wave): 4 columns each (K <= 128 in one pass)
constexpr int kRowsPerBlock = kHB / kRowLanes;
constexpr int kWRows = 64;    // rows per block of the weight-gradient pass
constexpr int kMaxOut = 4;    // head outputs (act_dim <= 4)
constexpr int kMaxK = 255;    // hidden width (the weight pass keeps >= 3 row lanes of column quads)

// choose_action's exploration noise (agent.py:350-370, GaussianActionNoise
// :520-539, np.random.normal(0, sigma)): N(0,1) pairs by Box-Muller on one
// Philox2x32-10 block per (call, row, output pair), counter (step, row pair
// index), key from the seed; f32 log / sqrt / sincospi on 24-bit uniforms
// (u1 in (0, 1]).  Independent across rows, outputs and calls.
__device__ __forceinline__ float2 explore_normals(uint64_t seed, uint64_t step, int64_t row, int pair) {
    const uint32_t key = (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu) ^ ((uint32_t)(step >> 32) * 0xC2B2AE35u);
    const U2 r = philox2x32((uint32_t)step, (uint32_t)(row * 2 + pair), key);
    const float u1 = ((float)(r.x >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    return make_float2(rad * cs, rad * sn);
}

// sum over the 32 lanes of a half-wave (fixed tree); every lane gets it
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = kRowLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// z[j] = b[j] + sum_k h[k] W[j][k] for the row of this half-wave: lane l
// takes columns 4l..4l+3 (+128, +256 ...), then a half-wave sum
template <int NOUT>
__device__ __forceinline__ void row_dot_of(const float *h, const float *W, const float *b, int32_t K, int64_t row,
                                           int l, float (&z)[NOUT]) {
    const float *hr = h + row * K;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) z[j] = 0.0f;
    for (int k = 4 * l; k < K; k += 4 * kRowLanes) {
        float x[4];
        if ((K & 3) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(hr + k);
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = k + i < K ? hr[k + i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NOUT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < K) z[j] = fmaf(x[i], W[(size_t)j * K + k + i], z[j]);
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) z[j] = half_sum(z[j]) + b[j];  // addmm: bias added to the product
}

// Actor.forward's last line (agent.py:56-61) on one head output z: t = tanh(z), the action
// 0.5*(high-low) * t + 0.5*(high+low) with scale / shift those two constants of the output
__device__ __forceinline__ float actor_action(float z, float scale, float shift, float &t) {
    t = tanhf(z);
    return scale * t + shift;
}

// dh[row] = dz W (lane l: columns 4l..4l+3, +128 ...), zero where dh_mask <= 0 (dh_mask may be null)
template <int NOUT>
__device__ __forceinline__ void write_dh_of(float *dh, const float *W, const float *dh_mask, int32_t K, int64_t row,
                                            int l, const float (&dz)[NOUT]) {
    float *o = dh + row * K;
    for (int k = 4 * l; k < K; k += 4 * kRowLanes) {
        float r4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < NOUT; ++j)
                if (k + i < K) s = fmaf(dz[j], W[(size_t)j * K + k + i], s);
            r4[i] = dh_mask && k + i < K && !(dh_mask[row * K + k + i] > 0.0f) ? 0.0f : s;
        }
        if ((K & 3) == 0) {
            *reinterpret_cast<float4 *>(o + k) = make_float4(r4[0], r4[1], r4[2], r4[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < K) o[k + i] = r4[i];
        }
    }
}

// deterministic block sum (fixed shuffle tree per wave, waves in order); thread 0 gets it
__device__ __forceinline__ float block_sum(float v) {
    __shared__ float ws[kHB / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.0f;
    if (threadIdx.x == 0)
        for (int w = 0; w < kHB / 64; ++w) s += ws[w];
    return s;
}

template <class F>
hipError_t with_nout(int nout, F f) {
    switch (nout) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
}

unsigned row_blocks(int32_t B) { return (unsigned)((B + kRowsPerBlock - 1) / kRowsPerBlock); }

bool bad_shape(int32_t B, int32_t K, int32_t nout) { return B <= 0 || K <= 0 || K > kMaxK || nout <= 0 || nout > kMaxOut; }

int fail_arg(const char *fn) { return f110_set_error(F110_E_INVALID, std::string(fn) + ": bad arguments"); }

}  // namespace
}  // namespace f110
