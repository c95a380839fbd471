// f110_selfplay.hip — what a policy-driven opponent needs on the device (include/f110.h,
// "self-play"): the flat observation from any agent's seat (f110_agent_obs) and the actor's output
// layer written into a masked, strided set of action rows (f110_policy_head_rows).
//
// k_agent_obs is a pure copy with one f32 divide per scan entry: a thread moves one 16-byte quad
// (or one float on the scalar path) of an output row, consecutive threads consecutive quads, so
// both the scan read and the obs write are coalesced 16-B accesses.  The 4-float pose groups are
// quads of their own (B % 4 == 0 on the quad path), copied from the step's obs row in the seat's
// order.  No LDS, no atomics; every output element has one writer.
//
// k_policy_head_rows is k_head_fwd's actor epilogue (f110_ddpg.hip) on the shared row code of
// f110_head_rows.h: the same dot product, tanh and affine map, so an unmasked row carries the bits of
// f110_ddpg_actor_head's act.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/f110.h"
#include "f110_env_rows.h"
#include "f110_head_rows.h"
#include "f110_host_util.h"
#include "f110_step_args.h"

namespace f110 {
namespace {

struct AgentObsArgs {
    const float *scans, *obs;
    float *out;
    int64_t scan_env_stride, obs_stride, out_stride, n_envs;
    int32_t A, B, agent;
    float lmax;
};

// the pose group of the input row that output group g holds: the seat's own first, then the others ascending
__device__ __forceinline__ int seat_group(int g, int agent) { return g == 0 ? agent : (g <= agent ? g - 1 : g); }

// VEC: one float4 per thread (B % 4 == 0, strides % 4 == 0, 16-B aligned pointers); else one float
template <bool VEC>
__global__ void __launch_bounds__(kHB) k_agent_obs(AgentObsArgs a) {
    constexpr int kW = VEC ? 4 : 1;
    const int64_t per_row = ((int64_t)a.B + 4 * a.A) / kW;  // threads per output row
    const int64_t idx = (int64_t)blockIdx.x * kHB + threadIdx.x;
    if (idx >= a.n_envs * per_row) return;
    const int64_t e = idx / per_row;
    const int32_t j = (int32_t)(idx - e * per_row) * kW;  // first float of this thread in the row
    float *o = a.out + e * a.out_stride + j;
    if (j < a.B) {
        const float *s = a.scans + e * a.scan_env_stride + (int64_t)a.agent * a.B + j;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4 *>(s);
            *reinterpret_cast<float4 *>(o) = make_float4(obs_scan_value(v.x, a.lmax), obs_scan_value(v.y, a.lmax),
                                                         obs_scan_value(v.z, a.lmax), obs_scan_value(v.w, a.lmax));
        } else {
            *o = obs_scan_value(*s, a.lmax);
        }
    } else {
        const int g = (j - a.B) >> 2, c = (j - a.B) & 3;  // (VEC: c == 0)
        const float *p = a.obs + e * a.obs_stride + a.B + 4 * seat_group(g, a.agent) + c;
        if (VEC) *reinterpret_cast<float4 *>(o) = *reinterpret_cast<const float4 *>(p);
        else *o = *p;
    }
}

struct PolicyHeadArgs {
    const float *h, *W, *b, *scale, *shift;
    const uint8_t *row_mask;
    float *out;
    int64_t out_stride;
    int32_t B, K;
};

// one row per half-wave (k_head_fwd's geometry), the epilogue on its lane 0; masked rows do nothing
template <int NOUT>
__global__ void __launch_bounds__(kHB) k_policy_head_rows(PolicyHeadArgs a) {
    const int l = threadIdx.x & (kRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kRowLanes);
    if (row >= a.B || (a.row_mask && a.row_mask[row] == 0)) return;  // uniform per half-wave
    float z[NOUT];
    row_dot_of<NOUT>(a.h, a.W, a.b, a.K, row, l, z);
    if (l == 0) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            float t;
            a.out[row * a.out_stride + j] = actor_action(z[j], a.scale[j], a.shift[j], t);
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace f110

using namespace f110;

extern "C" int f110_agent_obs(const float *scans, int64_t scan_env_stride, const float *obs, int64_t obs_stride,
                              int64_t n_envs, int32_t n_agents, int32_t n_beams, int32_t agent, float lidar_max,
                              float *out, int64_t out_stride, void *stream) {
    if (agent_obs_bad_args(scans, scan_env_stride, obs, obs_stride, n_envs, n_agents, n_beams, agent, out, out_stride))
        return fail(F110_E_INVALID, "f110_agent_obs: bad arguments");
    AgentObsArgs a{};
    a.scans = scans, a.obs = obs, a.out = out;
    a.scan_env_stride = scan_env_stride, a.obs_stride = obs_stride, a.out_stride = out_stride, a.n_envs = n_envs;
    a.A = n_agents, a.B = n_beams, a.agent = agent, a.lmax = lidar_max;
    const bool vec = (n_beams & 3) == 0 && ((scan_env_stride | obs_stride | out_stride) & 3) == 0 && aligned16(scans) &&
                     aligned16(obs) && aligned16(out);
    const int64_t threads = n_envs * (((int64_t)n_beams + 4 * n_agents) / (vec ? 4 : 1));
    const int64_t blocks = (threads + kHB - 1) / kHB;
    if (blocks > 0x7fffffff) return fail(F110_E_INVALID, "f110_agent_obs: too many rows for one launch");
    if (vec) hipLaunchKernelGGL(k_agent_obs<true>, dim3((unsigned)blocks), dim3(kHB), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_agent_obs<false>, dim3((unsigned)blocks), dim3(kHB), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail("f110_agent_obs", e);
}

extern "C" int f110_policy_head_rows(const float *h, const float *W, const float *b, const float *scale,
                                     const float *shift, int64_t n_rows, int32_t K, int32_t nout,
                                     const uint8_t *row_mask, float *out, int64_t out_stride, void *stream) {
    if (n_rows > 0x7fffffff || bad_shape((int32_t)n_rows, K, nout) || !h || !W || !b || !scale || !shift || !out ||
        out_stride < nout)
        return fail_arg("f110_policy_head_rows");
    PolicyHeadArgs a{};
    a.h = h, a.W = W, a.b = b, a.scale = scale, a.shift = shift, a.row_mask = row_mask, a.out = out;
    a.out_stride = out_stride, a.B = (int32_t)n_rows, a.K = K;
    hipError_t e = with_nout(nout, [&](auto N) {
        hipLaunchKernelGGL(k_policy_head_rows<decltype(N)::value>, dim3(row_blocks(a.B)), dim3(kHB), 0,
                           (hipStream_t)stream, a);
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : hip_fail("f110_policy_head_rows", e);
}
