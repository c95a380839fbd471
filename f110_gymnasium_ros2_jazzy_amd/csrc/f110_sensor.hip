// f110_sensor.hip — the sensor randomization on the device (f110_sensor_apply, include/f110.h
// "sensor randomization"): a full observation row's B range columns scaled, noised, quantized,
// dropped and blacked out, its pose columns noised, under parameters drawn per env and episode; the
// collision columns and the tail carried through.  No reference counterpart (the reference's scan
// noise is one std for every env).  The row rule is f110_sensor.h's, which f110_host_sensor_apply
// states on the host.
//
//   k_sensor        one 256-thread block (four waves) per env.  Everything per env -- the counters,
//                   the key, the drawn parameter row, the mask byte -- depends on blockIdx alone, so
//                   it sits in scalar registers and the parameter row is one scalar load; an episode
//                   start redraws the row in every thread alike (three Philox blocks).  Thread t then
//                   takes columns t, t + 256, ...: one coalesced 4-byte load, one Philox4x32-10 block
//                   where the row needs a draw (no noise and no dropout: none), the rule, one
//                   coalesced store.  A column is read and written by the same thread, so out may be
//                   rows itself; then the untouched columns are not copied.  A masked-off env copies
//                   its row (or does nothing in place) and keeps counting.  Thread 0 stores the
//                   counters (and a redrawn row) behind a barrier every wave reaches after it has
//                   read them.  Every output column, parameter row and counter has one writer.
//                   A block per env rather than a flat grid over columns: the counters and the
//                   parameter row are read and written in the same launch, and with several
//                   workgroups per env their update would need a second launch or a grid hand-off.
//                   Four waves per env rather than one (as k_scan_obs has): a row of 1088 columns is
//                   then five dependent load-compute-store rounds per wave, not seventeen, with
//                   twice the waves in flight (measured: docs/DESIGN_HISTORY.md §3.31).
//   k_sensor_reset  one thread per env: episode = -1, step = 0 where the mask is set (or everywhere).
//
// No LDS, no atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_sensor.h"
#include "f110_task_args.h"

namespace f110 {

namespace {

__global__ void __launch_bounds__(kSensorThreads) k_sensor(SensorArgs a) {
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;  // (the grid is E blocks)
    int32_t episode = a.episode[e], step = a.step[e];
    const bool start = sensor_advance(episode, step, a.reset ? a.reset[e] : 0);
    const SensorKey key = sensor_key(a.seed, (uint64_t)(a.env_offset + e));
    SensorRow *held = reinterpret_cast<SensorRow *>(a.param_rows) + e;
    const SensorRow r = start ? sensor_draw_row(key, (uint32_t)episode, a.p, a.B, a.range_max) : *held;
    const bool on = !a.mask || a.mask[e] != 0;
    const float *row = a.rows + e * a.row_stride;
    float *o = a.out + e * a.out_stride;
    const bool in_place = o == row;
    const int32_t B = a.B, M = a.M, W = a.B + a.M + a.T;
    if (on) {
        const bool draws = sensor_beam_draws(r);
        for (int32_t b = tid; b < B; b += kSensorThreads) {
            U4 k{0u, 0u, 0u, 0u};
            if (draws) k = sensor_block(key, (uint32_t)episode, (uint32_t)step, (uint32_t)b);
            o[b] = sensor_beam(row[b], b, r, k);
        }
        for (int32_t m = tid; m < M; m += kSensorThreads) {
            U4 k{0u, 0u, 0u, 0u};
            const bool touched = sensor_pose_draws(r, m);
            if (touched) k = sensor_block(key, (uint32_t)episode, (uint32_t)step, (uint32_t)(B + m));
            if (touched || !in_place) o[B + m] = sensor_pose(row[B + m], m, r, k);
        }
    }
    if (!in_place)  // the tail, or a masked-off env's whole row
        for (int32_t c = (on ? B + M : 0) + tid; c < W; c += kSensorThreads) o[c] = row[c];
    __syncthreads();  // every wave has the counters and the held row in registers (no wave has left)
    if (tid == 0) {
        a.episode[e] = episode;
        a.step[e] = step;
        if (start) *held = r;
    }
}

__global__ void __launch_bounds__(256) k_sensor_reset(int32_t *episode, int32_t *step, const uint8_t *env_mask,
                                                      int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E && (!env_mask || env_mask[e])) {
        episode[e] = -1;
        step[e] = 0;
    }
}

}  // namespace

hipError_t launch_sensor(const SensorArgs &a, hipStream_t s) {
    if (a.E <= 0) return hipSuccess;
    if (a.E > 0x7fffffff || a.B > kSensorMaxBeams) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sensor, dim3((unsigned)a.E), dim3(kSensorThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sensor_reset(int32_t *episode, int32_t *step, const uint8_t *env_mask, int64_t E, hipStream_t s) {
    if (E <= 0) return hipSuccess;
    const int64_t blocks = (E + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sensor_reset, dim3((unsigned)blocks), dim3(256), 0, s, episode, step, env_mask, E);
    return hipGetLastError();
}

}  // namespace f110
