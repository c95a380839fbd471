// f110_scan_obs.hip — the compact LiDAR observation on the device (f110_scan_obs_push,
// include/f110.h "scan observation"): a full observation row's B range columns pooled into K
// sectors, the last F pooled frames stacked S pushes apart out of a per-env ring, the middle and
// tail columns carried through.  No reference counterpart (_pack_flat_obs hands the policy every
// range).  The row rule is f110_scan_obs.h's, which f110_host_scan_obs_push states on the host.
//
//   k_scan_obs        one wave per env, four envs per 256-thread block, as k_track_obs.  The wave
//                     loads its row's B columns into its own stretch of LDS, lane-consecutive: as
//                     float4 where the rows are 16-byte aligned and row_stride % 4 == 0 (the
//                     launcher decides, the stride is the caller's), as single floats otherwise.
//                     After the barrier lane l pools bins l, l + 64, ... from LDS, each in the
//                     rule's fixed beam order (one lane per bin is what keeps that order), and for
//                     its bin k writes the ring slot (all D slots on a refill), column k of frame 0
//                     from the register, and columns j*K + k of frames 1..F-1 from the ring's slot
//                     (head - j*S) mod D: a slot other than the one just written whenever D > 1,
//                     and the same lane's own column, so no lane waits for another's store.  All
//                     of these are lane-consecutive over k.  The middle and tail columns go
//                     straight from the input row to the output row.  Lane 0 stores the new head.
//                     Every output column, ring word and head has one writer.
//   k_scan_obs_reset  one thread per env: head = -1 where the mask is set (or everywhere).
//
// LDS: 4 * round_up(B, 4) floats per block (17 KiB at B = 1080; B <= 4096 keeps it within 64 KiB).
// A bin's beams are B/K apart between neighbouring lanes: a 2-way bank conflict on the ds_read_b32
// at the strides 10 (K = 108) and 30 (K = 36), on a kernel that is bound by the row's global load.
// No atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_scan_obs.h"
#include "f110_task_args.h"

namespace f110 {

namespace {

__global__ void __launch_bounds__(64 * kScanObsEnvs) k_scan_obs(ScanObsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * kScanObsEnvs + w;
    const bool live = e < a.E;  // the whole wave
    const int32_t B = a.B, K = a.K;
    float *v = lds + (size_t)w * ((B + 3) & ~3);
    const float *row = a.rows + (live ? e : 0) * a.row_stride;
    if (live) {
        if (a.vec4) {
            const float4 *r4 = reinterpret_cast<const float4 *>(row);
            float4 *v4 = reinterpret_cast<float4 *>(v);
            for (int32_t i = lane; i < B / 4; i += 64) v4[i] = r4[i];
            const int32_t t = (B & ~3) + lane;  // the last B % 4 columns
            if (t < B) v[t] = row[t];
        } else {
            for (int32_t i = lane; i < B; i += 64) v[i] = row[i];
        }
    }
    __syncthreads();  // (every wave of the block arrives: none has left)
    if (!live) return;
    const int32_t D = a.D, F = a.F, S = a.S;
    bool refill;
    const int32_t h = scan_obs_advance(a.head[e], a.reset ? a.reset[e] : 0, D, refill);
    float *rg = a.ring + e * D * K;
    float *o = a.out + e * a.out_stride;
    for (int32_t k = lane; k < K; k += 64) {
        const float p = scan_obs_pool(v, scan_obs_edge(k, B, K), scan_obs_edge(k + 1, B, K), a.reduce);
        if (refill) {
            for (int32_t d = 0; d < D; ++d) rg[(int64_t)d * K + k] = p;
        } else {
            rg[(int64_t)h * K + k] = p;
        }
        o[k] = p;
        for (int32_t j = 1; j < F; ++j)
            o[(int64_t)j * K + k] = refill ? p : rg[(int64_t)scan_obs_slot(h, j, S, D) * K + k];
    }
    const int32_t skip = a.keep_mid ? 0 : a.M, n_copy = a.M + a.T - skip;
    for (int32_t c = lane; c < n_copy; c += 64) o[(int64_t)F * K + c] = row[B + skip + c];
    if (lane == 0) a.head[e] = h;
}

__global__ void __launch_bounds__(256) k_scan_obs_reset(int32_t *head, const uint8_t *env_mask, int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E && (!env_mask || env_mask[e])) head[e] = -1;
}

}  // namespace

hipError_t launch_scan_obs(const ScanObsArgs &a, hipStream_t s) {
    if (a.E <= 0) return hipSuccess;
    const int64_t blocks = (a.E + kScanObsEnvs - 1) / kScanObsEnvs;
    if (blocks > 0x7fffffff || a.B > kScanObsMaxBeams) return hipErrorInvalidValue;
    const size_t lds = (size_t)kScanObsEnvs * ((a.B + 3) & ~3) * sizeof(float);
    hipLaunchKernelGGL(k_scan_obs, dim3((unsigned)blocks), dim3(64 * kScanObsEnvs), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_scan_obs_reset(int32_t *head, const uint8_t *env_mask, int64_t E, hipStream_t s) {
    if (E <= 0) return hipSuccess;
    const int64_t blocks = (E + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_obs_reset, dim3((unsigned)blocks), dim3(256), 0, s, head, env_mask, E);
    return hipGetLastError();
}

}  // namespace f110
