// f110_td3.hip — the TD3 learner's heads (include/f110.h, "TD3 heads"): the target actor's output
// layer with target-policy smoothing, and the twin critics' TD-target / loss / backward head in
// one launch.  Same launch shape as f110_ddpg.hip's heads (f110_head_rows.h: one row per
// half-wave, the epilogue in registers, deterministic block sums); the per-row arithmetic is
// td3_smooth_one / td3_row (f110_head_rows.h), which the host hooks of this file run too.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_head_rows.h"
#include "f110_host_util.h"

namespace f110 {
namespace {

// xor-ed into the seed of explore_normals: the smoothing stream never coincides with the
// exploration stream of the same (seed, counter, row)
constexpr uint64_t kSmoothTag = 0x5444335F534D5448ull;  // "TD3_SMTH"

struct Td3Args {
    // target action: the target actor's last hidden layer and head, its affine map and the box
    const float *h, *W, *b;
    const float *scale, *shift, *lo, *hi;
    const float *normals_ext;  // [B][nout] caller-supplied N(0,1), or null: the device stream
    const int64_t *counter;    // device word, read only (the critic optimizer's step)
    float *out;                // [B][nout]
    float policy_noise, noise_clip;
    uint64_t seed;
    // critic step: the two target critics (t) and the two critics, last hidden layers and heads
    const float *ht1, *Wt1, *bt1, *ht2, *Wt2, *bt2;
    const float *h1, *W1, *b1, *h2, *W2, *b2;
    const float *r, *d, *w, *g;
    float *td, *dq1, *dq2;     // td: the PER priority 0.5 (|td1| + |td2|); dq_i may be null
    float *dh1, *dh2;          // dq_i W_i where dh_i_mask > 0 (each may be null)
    const float *dh1_mask, *dh2_mask;
    float *part;               // [row_blocks(B)] block sums of w td1^2 + w td2^2
    float gamma;
    int32_t B, K, nout;
};

// the target actor's head (k_head_fwd kActor's act, bit for bit) + td3_smooth_one on lane 0
template <int NOUT>
__global__ void __launch_bounds__(kHB) k_td3_target_action(Td3Args a) {
    const int l = threadIdx.x & (kRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
    if (row >= a.B) return;  // uniform per half-wave
    float z[NOUT];
    row_dot_of<NOUT>(a.h, a.W, a.b, a.K, row, l, z);
    if (l != 0) return;
    const uint64_t step = a.normals_ext ? 0 : (uint64_t)*a.counter;
#pragma unroll
    for (int j = 0; j < NOUT; j += 2) {
        float2 nz = make_float2(0.0f, 0.0f);
        if (a.normals_ext) {
            nz.x = a.normals_ext[row * NOUT + j];
            if (j + 1 < NOUT) nz.y = a.normals_ext[row * NOUT + j + 1];
        } else {
            nz = explore_normals(a.seed ^ kSmoothTag, step, row, j >> 1);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (j + q >= NOUT) break;
            const float act = a.scale[j + q] * tanhf(z[j + q]) + a.shift[j + q];
            a.out[row * NOUT + j + q] = td3_smooth_one(act, q == 0 ? nz.x : nz.y, a.policy_noise, a.noise_clip,
                                                       a.scale[j + q], a.lo[j + q], a.hi[j + q]);
        }
    }
}

// k_critic_step's twin: per row (one half-wave) the four critic heads, td3_row, and each
// critic's dh = dq_i W_i where its mask > 0; the block sums of the row loss terms
__global__ void __launch_bounds__(kHB) k_td3_critic_step(Td3Args a) {
    const int l = threadIdx.x & (kRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
    float v = 0.0f;
    if (row < a.B) {
        float q1t[1], q2t[1], q1[1], q2[1];
        row_dot_of<1>(a.ht1, a.Wt1, a.bt1, a.K, row, l, q1t);
        row_dot_of<1>(a.ht2, a.Wt2, a.bt2, a.K, row, l, q2t);
        row_dot_of<1>(a.h1, a.W1, a.b1, a.K, row, l, q1);
        row_dot_of<1>(a.h2, a.W2, a.b2, a.K, row, l, q2);
        const float gb = *a.g / (float)a.B;
        float td1, td2, dq1, dq2, prio, wl;  // every lane: write_dh needs dq_i
        td3_row(a.r[row], a.d[row], a.gamma, q1t[0], q2t[0], q1[0], q2[0], a.w[row], gb, td1, td2, dq1, dq2, prio,
                wl);
        if (l == 0) {
            a.td[row] = prio;
            v = wl;
            if (a.dq1) a.dq1[row] = dq1;
            if (a.dq2) a.dq2[row] = dq2;
        }
        const float dz1[1] = {dq1}, dz2[1] = {dq2};
        if (a.dh1) write_dh_of<1>(a.dh1, a.W1, a.dh1_mask, a.K, row, l, dz1);
        if (a.dh2) write_dh_of<1>(a.dh2, a.W2, a.dh2_mask, a.K, row, l, dz2);
    }
    const float s = block_sum(v);
    if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}

bool bad_noise(float policy_noise, float noise_clip) {
    return !std::isfinite(policy_noise) || !std::isfinite(noise_clip) || policy_noise < 0.0f || noise_clip < 0.0f;
}

}  // namespace
}  // namespace f110

using namespace f110;

extern "C" int f110_td3_target_action(const float *h, const float *W, const float *b, const float *scale,
                                      const float *shift, int32_t B, int32_t K, int32_t nout, float policy_noise,
                                      float noise_clip, const float *low, const float *high, uint64_t seed,
                                      const int64_t *counter, const float *normals_ext, float *out, void *stream) {
    if (bad_shape(B, K, nout) || !h || !W || !b || !scale || !shift || !low || !high || !out ||
        bad_noise(policy_noise, noise_clip) || (!normals_ext && !counter))
        return fail_arg("f110_td3_target_action");
    Td3Args a{};
    a.h = h, a.W = W, a.b = b, a.scale = scale, a.shift = shift, a.lo = low, a.hi = high;
    a.normals_ext = normals_ext, a.counter = counter, a.out = out;
    a.policy_noise = policy_noise, a.noise_clip = noise_clip, a.seed = seed;
    a.B = B, a.K = K, a.nout = nout;
    hipError_t e = with_nout(nout, [&](auto N) {
        hipLaunchKernelGGL(k_td3_target_action<decltype(N)::value>, dim3(row_blocks(B)), dim3(kHB), 0,
                           (hipStream_t)stream, a);
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : hip_fail("f110_td3_target_action", e);
}

extern "C" int f110_td3_critic_step(const float *ht1, const float *Wt1, const float *bt1, const float *ht2,
                                    const float *Wt2, const float *bt2, const float *r, const float *d, float gamma,
                                    const float *h1, const float *W1, const float *b1, const float *h2,
                                    const float *W2, const float *b2, const float *w, const float *g, int32_t B,
                                    int32_t K, float *td, float *dh1, const float *dh1_mask, float *dh2,
                                    const float *dh2_mask, float *dq1, float *dq2, float *part, void *stream) {
    if (bad_shape(B, K, 1) || !ht1 || !Wt1 || !bt1 || !ht2 || !Wt2 || !bt2 || !r || !d || !h1 || !W1 || !b1 || !h2 ||
        !W2 || !b2 || !w || !g || !td || !part)
        return fail_arg("f110_td3_critic_step");
    Td3Args a{};
    a.ht1 = ht1, a.Wt1 = Wt1, a.bt1 = bt1, a.ht2 = ht2, a.Wt2 = Wt2, a.bt2 = bt2;
    a.h1 = h1, a.W1 = W1, a.b1 = b1, a.h2 = h2, a.W2 = W2, a.b2 = b2;
    a.r = r, a.d = d, a.w = w, a.g = g, a.gamma = gamma;
    a.td = td, a.dq1 = dq1, a.dq2 = dq2, a.dh1 = dh1, a.dh2 = dh2, a.dh1_mask = dh1_mask, a.dh2_mask = dh2_mask;
    a.part = part;
    a.B = B, a.K = K, a.nout = 1;
    hipLaunchKernelGGL(k_td3_critic_step, dim3(row_blocks(B)), dim3(kHB), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail("f110_td3_critic_step", e);
}

extern "C" int f110_host_td3_smooth_rows(const float *act, const float *normals, int64_t n_rows, int32_t nout,
                                         float policy_noise, float noise_clip, const float *scale, const float *low,
                                         const float *high, float *out) {
    if (n_rows <= 0 || nout <= 0 || nout > kMaxOut || !act || !normals || !scale || !low || !high || !out ||
        bad_noise(policy_noise, noise_clip))
        return fail_arg("f110_host_td3_smooth_rows");
    for (int64_t r = 0; r < n_rows; ++r)
        for (int j = 0; j < nout; ++j) {
            const int64_t i = r * nout + j;
            out[i] = td3_smooth_one(act[i], normals[i], policy_noise, noise_clip, scale[j], low[j], high[j]);
        }
    return 0;
}

extern "C" int f110_host_td3_rows(const float *r, const float *d, float gamma, const float *q1t, const float *q2t,
                                  const float *q1, const float *q2, const float *w, float g, int64_t B, float *td1,
                                  float *td2, float *dq1, float *dq2, float *prio, float *wl) {
    if (B <= 0 || B > INT32_MAX || !r || !d || !q1t || !q2t || !q1 || !q2 || !w || !td1 || !td2 || !dq1 || !dq2 ||
        !prio || !wl)
        return fail_arg("f110_host_td3_rows");
    const float gb = g / (float)(int32_t)B;
    for (int64_t i = 0; i < B; ++i)
        td3_row(r[i], d[i], gamma, q1t[i], q2t[i], q1[i], q2[i], w[i], gb, td1[i], td2[i], dq1[i], dq2[i], prio[i],
                wl[i]);
    return 0;
}
